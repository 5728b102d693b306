"""-m gpu tests of multicolor_order / permute_inspect / permute / permute_vector (spblas_gfx950_multicolor_* / csr_permute_* /
permute_vector, csrc/multicolor.hip).  Every test fails on a backend without the feature: the names do not exist there.

Generators, the host model (sequential greedy in descending key order -- not the device's rounds) and the checkers:
tests/multicolor_util.py, proved on the host by tests/test_multicolor_cpu.py.  The device's colours must equal the model's BIT FOR
BIT and pass the independent validity check; the permuted structure and values must equal the host's bit for bit.  Every output
array is longer than its result and poisoned behind it."""
import gc

import numpy as np
import pytest
import torch

import gpu_util as G
import ilu_util as U
import multicolor_util as M
import spblas_reference_amd as sp

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
PAD = 5
WILD = 2 ** 30
FIXTURES = M.fixtures()
MODEL = {}           # name -> the model's colours, computed once


def model(name):
    if name not in MODEL:
        MODEL[name] = M.model_colors(*FIXTURES[name])
    return MODEL[name]


def on_device(rowptr, colind, values=None, dtype=np.float32):
    """csr_view over over-long arrays: a wild column and NaN behind nnz."""
    m, nnz = rowptr.size - 1, int(colind.size)
    v = np.ones(nnz) if values is None else np.asarray(values, np.float64)
    d_v = G.dev(np.concatenate([v, np.full(PAD, np.nan)]).astype(dtype))
    d_ci = G.dev(np.concatenate([colind.astype(np.int32), np.full(PAD, WILD, np.int32)]))
    return sp.csr_view(d_v, G.dev(rowptr.astype(np.int32)), d_ci, (m, m), nnz)


def empty_b(m, nnz, dtype):
    """B's arrays, poisoned throughout: rowptr / colind with WILD, values with NaN."""
    td = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    return sp.csr_view(torch.full((nnz + PAD,), float("nan"), dtype=td, device="cuda"),
                       torch.full((m + 1 + PAD,), WILD, dtype=torch.int32, device="cuda"),
                       torch.full((nnz + PAD,), WILD, dtype=torch.int32, device="cuda"), (m, m), nnz)


# ---- colouring ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_colours_equal_the_sequential_model_bit_for_bit(gpu, name):
    rowptr, colind = FIXTURES[name]
    m = rowptr.size - 1
    order = sp.multicolor_order(on_device(rowptr, colind))
    color, perm, inverse, color_ptr = (G.host(t) for t in (order.color, order.perm, order.inverse, order.color_ptr))
    want = model(name)
    assert color.dtype == np.int32 and np.array_equal(color, want), f"{int((color != want).sum())} colours differ from the model"
    assert M.check_order(rowptr, colind, color, perm, inverse, color_ptr) == []
    w_perm, w_inv, w_ptr = M.order_from_colors(want)
    assert np.array_equal(perm, w_perm) and np.array_equal(inverse, w_inv) and np.array_equal(color_ptr, w_ptr)
    info = order.info()
    assert info["colors"] == w_ptr.size - 1
    assert info["max_color_size"] == (int(np.diff(w_ptr).max()) if m else 0)
    assert info["lanes_per_row"] == M.lanes_for(rowptr, colind)
    assert (0 if m == 0 else 1) <= info["rounds"] <= m
    if name.startswith("complete_"):
        assert info["colors"] == m          # 65 and 130 colours: past the first and the second 64-colour window


def test_every_lane_count_is_taken(gpu):
    got = {sp.multicolor_order(on_device(*p)).info()["lanes_per_row"] for _, p in M.lane_patterns()}
    assert got == {4, 8, 16, 64}


def test_repeated_calls_give_identical_bits(gpu):
    for name in ("random_2000x6", "lap7_12", "slow_path_300"):
        a = on_device(*FIXTURES[name])
        first, second = sp.multicolor_order(a), sp.multicolor_order(a)
        for f in ("color", "perm", "inverse", "color_ptr"):
            assert torch.equal(getattr(first, f), getattr(second, f))


def test_copy_leaves_over_long_arrays_poisoned_behind_their_results(gpu):
    """The C entry point with caller arrays longer than m / colours + 1, and with NULL outputs."""
    from spblas_reference_amd import _capi
    import ctypes
    rowptr, colind = FIXTURES["grid5_9x7"]
    m = rowptr.size - 1
    a = on_device(rowptr, colind)
    hd = sp.api._Handle.current(a.rowptr().device)
    lib, plan = _capi.lib(), ctypes.c_void_p()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.spblas_gfx950_multicolor_create(hd.h, ctypes.byref(plan), m, a.size(), p(a.rowptr()), p(a.colind())) == 0
    try:
        arr = (ctypes.c_int64 * 4)()
        assert lib.spblas_gfx950_multicolor_info(plan, arr) == 0
        ncol = int(arr[0])
        outs = [torch.full((n + PAD,), WILD, dtype=torch.int32, device="cuda") for n in (m, m, m, ncol + 1)]
        assert lib.spblas_gfx950_multicolor_copy(hd.h, plan, *(p(t) for t in outs)) == 0
        assert lib.spblas_gfx950_multicolor_copy(hd.h, plan, None, None, None, None) == 0
        only = torch.full((m + PAD,), WILD, dtype=torch.int32, device="cuda")
        assert lib.spblas_gfx950_multicolor_copy(hd.h, plan, None, None, p(only), None) == 0
    finally:
        assert lib.spblas_gfx950_multicolor_destroy(hd.h, plan) == 0
    want = model("grid5_9x7")
    for t, n in zip(outs, (m, m, m, ncol + 1)):
        assert (G.host(t)[n:] == WILD).all(), "a copy wrote behind its result"
    assert np.array_equal(G.host(outs[2])[:m], want) and np.array_equal(G.host(only)[:m], want)
    assert (G.host(only)[m:] == WILD).all()


def test_structure_errors_are_value_errors(gpu):
    rowptr, colind = FIXTURES["grid5_9x7"]
    m = rowptr.size - 1
    bad = colind.copy()
    bad[7] = m                                              # a column >= m
    with pytest.raises(ValueError):
        sp.multicolor_order(on_device(rowptr, bad))
    bad[7] = -1
    with pytest.raises(ValueError):
        sp.multicolor_order(on_device(rowptr, bad))
    rp = rowptr.copy()
    rp[-1] -= 1                                             # offsets that do not describe nnz entries
    with pytest.raises(ValueError):
        sp.multicolor_order(on_device(rp, colind))
    rp = rowptr.copy()
    rp[3], rp[4] = rp[4], rp[3]                             # descending offsets
    with pytest.raises(ValueError):
        sp.multicolor_order(on_device(rp, colind))
    with pytest.raises(ValueError):
        sp.permute_inspect(on_device(rowptr, bad), G.dev(np.arange(m, dtype=np.int32)), empty_b(m, colind.size, np.float32))


def test_inspects_raise_inside_a_capture(gpu):
    rowptr, colind = FIXTURES["grid5_9x7"]
    m = rowptr.size - 1
    a = on_device(rowptr, colind)
    perm = G.dev(np.arange(m, dtype=np.int32))
    b = empty_b(m, colind.size, np.float32)
    x, y = torch.rand(m, device="cuda"), torch.zeros(m, device="cuda")
    sp.multicolor_order(a)                                  # the handle exists before the capture
    torch.cuda.synchronize()
    raised = []
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for call in (lambda: sp.multicolor_order(a), lambda: sp.permute_inspect(a, perm, b)):
            try:
                call()
                raised.append(None)
            except Exception as e:  # noqa: BLE001
                raised.append(e)
        sp.permute_vector(perm, x, y)                       # the execute-class call IS recordable
    assert all(isinstance(e, sp.BackendError) and "not supported" in str(e).lower() for e in raised), raised
    assert (G.host(b.rowptr()) == WILD).all()
    g.replay()
    assert torch.equal(y, x)
    assert sp.multicolor_order(a).info()["colors"] == int(model("grid5_9x7").max()) + 1     # and outside the capture everything works as before


# ---- permutation -------------------------------------------------------------------------------------------------------
PMATS = M.permutation_matrices()


def perms_for(name, rowptr, colind):
    m = rowptr.size - 1
    rng = np.random.default_rng(len(name))
    out = {"identity": np.arange(m, dtype=np.int32), "reversal": np.arange(m, dtype=np.int32)[::-1].copy(),
           "random": rng.permutation(m).astype(np.int32)}
    out["multicolor"] = M.order_from_colors(M.model_colors(rowptr, colind))[0]
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(PMATS))
def test_permuted_matrix_equals_the_hosts_bit_for_bit(gpu, name, dtype):
    rowptr, colind = PMATS[name]
    m, nnz = rowptr.size - 1, int(colind.size)
    vals = np.random.default_rng(2).standard_normal(nnz)
    a = on_device(rowptr, colind, vals, dtype)
    a_host = vals.astype(dtype)
    for pname, perm in perms_for(name, rowptr, colind).items():
        w_rp, w_ci, w_pos = M.host_permute(rowptr, colind, perm)
        b = empty_b(m, nnz, dtype)
        d_perm = G.dev(perm)
        sp.permute(a, d_perm, b)
        rp, ci, v = G.host(b.rowptr()), G.host(b.colind()), G.host(b.values())
        assert np.array_equal(rp[:m + 1], w_rp), (pname, "rowptr")
        assert np.array_equal(ci[:nnz], w_ci), (pname, "colind")
        assert np.array_equal(U.bits(v[:nnz]), U.bits(a_host[w_pos])), (pname, "values")
        assert (rp[m + 1:] == WILD).all() and (ci[nnz:] == WILD).all() and np.isnan(v[nnz:]).all(), "written behind the end"
        assert tuple(b.shape()) == (m, m) and b.size() == nnz
        if name != "duplicates":
            for i in range(m):
                assert (np.diff(ci[rp[i]:rp[i + 1]]) > 0).all(), "columns not strictly ascending"
        if pname == "identity" and name == "lap7_5x4x3":        # sorted rows: A's own arrays
            assert np.array_equal(rp[:m + 1], rowptr) and np.array_equal(ci[:nnz], colind)
            assert np.array_equal(U.bits(v[:nnz]), U.bits(a_host))
        assert np.array_equal(U.bits(G.host(a.values())[:nnz]), U.bits(a_host)), "A's values changed"


@pytest.mark.parametrize("dtype", DTYPES)
def test_info_form_refreshes_the_values_eagerly_and_in_a_graph(gpu, dtype):
    rowptr, colind = PMATS["duplicates"]
    m, nnz = rowptr.size - 1, int(colind.size)
    rng = np.random.default_rng(5)
    perm = rng.permutation(m).astype(np.int32)
    _, w_ci, w_pos = M.host_permute(rowptr, colind, perm)
    a = on_device(rowptr, colind, rng.standard_normal(nnz), dtype)
    b = empty_b(m, nnz, dtype)
    d_perm = G.dev(perm)
    info = sp.permute_inspect(a, d_perm, b)
    assert np.array_equal(G.host(b.colind())[:nnz], w_ci) and np.isnan(G.host(b.values())).all()   # structure only
    assert tuple(info.result_shape()) == (m, m) and info.result_nnz() == nnz
    plan = info.state_
    for _ in range(2):                                        # two refreshes after editing A's values in place
        new = rng.standard_normal(nnz).astype(dtype)
        a.values()[:nnz].copy_(G.dev(new))
        b.colind().fill_(WILD)                                # the info form must not touch the structure again
        sp.permute(info, a, d_perm, b)
        assert info.state_ is plan
        assert np.array_equal(U.bits(G.host(b.values())[:nnz]), U.bits(new[w_pos]))
        assert (G.host(b.colind()) == WILD).all()
    g = torch.cuda.CUDAGraph()
    b.values().fill_(float("nan"))
    with torch.cuda.graph(g):
        sp.permute(info, a, d_perm, b)
    for _ in range(2):
        new = rng.standard_normal(nnz).astype(dtype)
        a.values()[:nnz].copy_(G.dev(new))
        b.values().fill_(float("nan"))
        g.replay()
        v = G.host(b.values())
        assert np.array_equal(U.bits(v[:nnz]), U.bits(new[w_pos])) and np.isnan(v[nnz:]).all()
    # an info made for other arrays is replaced by a new inspect
    b2 = empty_b(m, nnz, dtype)
    sp.permute(info, a, d_perm, b2)
    assert info.state_ is not plan and np.array_equal(G.host(b2.colind())[:nnz], w_ci)


@pytest.mark.parametrize("what", ["repeated", "too_large", "negative"])
def test_a_wrong_perm_is_a_value_error_and_leaves_b_untouched(gpu, what):
    rowptr, colind = PMATS["distinct"]
    m, nnz = rowptr.size - 1, int(colind.size)
    perm = np.random.default_rng(6).permutation(m).astype(np.int32)
    perm[17] = {"repeated": perm[200], "too_large": m, "negative": -1}[what]
    a = on_device(rowptr, colind)
    for call in (sp.permute_inspect, sp.permute):
        b = empty_b(m, nnz, np.float32)
        with pytest.raises(ValueError):
            call(a, G.dev(perm), b)
        assert (G.host(b.rowptr()) == WILD).all() and (G.host(b.colind()) == WILD).all() and np.isnan(G.host(b.values())).all()


def test_values_call_checks_its_plan_and_its_buffers(gpu):
    from spblas_reference_amd import _capi
    rowptr, colind = PMATS["lap7_5x4x3"]
    m, nnz = rowptr.size - 1, int(colind.size)
    a, b = on_device(rowptr, colind), empty_b(m, nnz, np.float32)
    info = sp.permute_inspect(a, G.dev(np.arange(m, dtype=np.int32)), b)
    plan, lib = info.state_, _capi.lib()
    av, bv = a.values().data_ptr(), b.values().data_ptr()
    call = lambda n, x, y, vt: lib.spblas_gfx950_csr_permute_values(plan.hd.h, plan.plan, n, x, y, vt)
    assert call(nnz - 1, av, bv, _capi.F32) == _capi.PLAN_MISMATCH
    assert call(nnz, av, av, _capi.F32) == _capi.INVALID_VALUE          # no in-place form
    assert call(nnz, av, bv, 99) == _capi.INVALID_VALUE
    assert call(nnz, av, bv, _capi.C32) == _capi.NOT_SUPPORTED
    assert call(nnz, None, bv, _capi.F32) == _capi.INVALID_POINTER
    assert call(nnz, av, bv, _capi.F32) == _capi.SUCCESS
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_permute_vector_forward_then_inverse_matches_torch_indexing(gpu, dtype):
    td = torch.float32 if dtype == np.float32 else torch.float64
    for n in (0, 1, 255, 4097):
        perm = torch.randperm(n, device="cuda").to(torch.int32)
        src = torch.randn(n + PAD, dtype=td, device="cuda")[:n]
        fwd_buf = torch.full((n + PAD,), float("nan"), dtype=td, device="cuda")
        back_buf = torch.full((n + PAD,), float("nan"), dtype=td, device="cuda")
        sp.permute_vector(perm, src, fwd_buf[:n])
        assert torch.equal(fwd_buf[:n], src[perm.long()])
        sp.permute_vector(perm, fwd_buf[:n], back_buf[:n], inverse=True)
        assert torch.equal(back_buf[:n], src)
        assert torch.isnan(fwd_buf[n:]).all() and torch.isnan(back_buf[n:]).all()
    x = torch.ones(4, dtype=td, device="cuda")
    with pytest.raises(ValueError):
        sp.permute_vector(torch.arange(4, dtype=torch.int32, device="cuda"), x, x)


def test_complex_and_16_bit_values_raise_type_error(gpu):
    rowptr, colind = PMATS["lap7_5x4x3"]
    m, nnz = rowptr.size - 1, int(colind.size)
    perm = G.dev(np.arange(m, dtype=np.int32))
    for td in (torch.complex64, torch.complex128, torch.float16, torch.bfloat16):
        mk = lambda: sp.csr_view(torch.ones(nnz, dtype=td, device="cuda"), G.dev(rowptr), G.dev(colind), (m, m), nnz)
        with pytest.raises(TypeError):
            sp.multicolor_order(mk())
        with pytest.raises(TypeError):
            sp.permute(mk(), perm, mk())
        with pytest.raises(TypeError):
            sp.permute_inspect(mk(), perm, mk())
        with pytest.raises(TypeError):
            sp.permute_vector(perm, torch.ones(m, dtype=td, device="cuda"), torch.ones(m, dtype=td, device="cuda"))


def test_create_use_destroy_cycles_do_not_leak_device_memory(gpu):
    rowptr, colind = M.laplacian7(40, 40, 40)
    m, nnz = rowptr.size - 1, int(colind.size)
    a = on_device(rowptr, colind)
    b = empty_b(m, nnz, np.float32)
    x, y = torch.rand(m, device="cuda"), torch.zeros(m, device="cuda")

    def cycle():
        order = sp.multicolor_order(a)
        info = sp.permute_inspect(a, order.perm, b)
        sp.permute(info, a, order.perm, b)
        sp.permute_vector(order.perm, x, y)
        del order, info
        torch.cuda.synchronize()
        gc.collect()

    for _ in range(4):      # warm-up: pools and the handle's scratch reach their size
        cycle()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(25):
        cycle()
    free1, _ = torch.cuda.mem_get_info()
    lost = free0 - free1
    # one cycle allocates ~10 MB of plans and work arrays: a leak of any of them shows over 25 cycles
    assert lost < 8 * 2 ** 20, f"free device memory fell by {lost / 2**20:.1f} MiB over 25 cycles"


# ---- pairing with ilu0 and the solves, on the 12^3 Laplacian -----------------------------------------------------------------
@pytest.fixture(scope="module")
def lap12(gpu):
    rowptr, colind = FIXTURES["lap7_12"]
    m, nnz = rowptr.size - 1, int(colind.size)
    a = on_device(rowptr, colind)
    order = sp.multicolor_order(a)
    perm = G.host(order.perm)
    assert np.array_equal(perm, M.order_from_colors(model("lap7_12"))[0])
    b_rp, b_ci, pos = M.host_permute(rowptr, colind, perm)
    return dict(rowptr=rowptr, colind=colind, m=m, nnz=nnz, order=order, perm=perm, b_rp=b_rp, b_ci=b_ci, pos=pos)


def test_level_plans_of_the_permuted_matrix_are_as_shallow_as_the_colouring(lap12):
    L = lap12
    colours = L["order"].info()["colors"]
    assert colours == 6
    a = on_device(L["rowptr"], L["colind"])
    b = empty_b(L["m"], L["nnz"], np.float32)
    sp.permute(a, L["order"].perm, b)
    v, w = torch.zeros(L["m"], device="cuda"), torch.zeros(L["m"], device="cuda")
    tri = [(sp.lower_triangle, sp.implicit_unit_diagonal), (sp.upper_triangle, sp.explicit_diagonal)]
    for t in tri:
        assert sp.triangular_solve_inspect(a, *t, v, w).state_.info()["levels"] == 34
        assert sp.triangular_solve_inspect(b, *t, v, w).state_.info()["levels"] <= colours
    assert sp.ilu0_inspect(a).state_.info()["levels"] == 34
    assert sp.ilu0_inspect(b).state_.info()["levels"] <= colours


@pytest.mark.parametrize("dtype", DTYPES)
def test_ilu0_and_both_solves_on_the_permuted_matrix(lap12, dtype):
    """The exact family of tests/ilu_util.py on B's pattern: A's values are B's taken back to A's order, so the device must
    deliver B's values, the factor `want` and -- with P b = L (U x) in float64 for a dyadic x -- the solution, all bit for bit
    (the bound of test_gpu_ilu0.py's solve check: equality), after the result is taken back to A's order.  Random dominant values
    then pass ilu_util.residual_violations, that file's own bound for inexact data."""
    L = lap12
    m, nnz, pos, perm = L["m"], L["nnz"], L["pos"], L["perm"]
    b_vals, want = U.exact_system(L["b_rp"], L["b_ci"], seed=31)
    a_vals = np.empty(nnz)
    a_vals[pos] = b_vals
    a = on_device(L["rowptr"], L["colind"], a_vals, dtype)
    b = empty_b(m, nnz, dtype)
    pinfo = sp.permute_inspect(a, L["order"].perm, b)
    sp.permute(pinfo, a, L["order"].perm, b)
    assert np.array_equal(G.host(b.rowptr())[:m + 1], L["b_rp"]) and np.array_equal(G.host(b.colind())[:nnz], L["b_ci"])
    assert np.array_equal(U.bits(G.host(b.values())[:nnz]), U.bits(b_vals.astype(dtype)))
    td = b.values().dtype
    lu = sp.csr_view(torch.full((nnz + PAD,), float("nan"), dtype=td, device="cuda"), b.rowptr(), b.colind(), (m, m), nnz)
    info = sp.ilu0_inspect(b)
    sp.ilu0(info, b, lu)
    assert sp.ilu0_status(info) == -1
    assert U.exact_violations(G.host(lu.values())[:nnz], want, L["b_rp"], L["b_ci"]) == []
    # the solves: x in B's order is dyadic, b = L (U x) exact in float64; both live in A's order on the device
    Lm, Um = U.split_lu(L["b_rp"], L["b_ci"], want)
    px_true = np.random.default_rng(7).choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], m)
    pb = Lm @ (Um @ px_true)
    rhs, x_true = np.empty(m), np.empty(m)
    rhs[perm], x_true[perm] = pb, px_true
    nan = lambda: torch.full((m,), float("nan"), dtype=td, device="cuda")
    d_rhs, d_pb, d_y, d_px, d_x = G.dev(rhs.astype(dtype)), nan(), nan(), nan(), nan()
    sp.permute_vector(L["order"].perm, d_rhs, d_pb)
    sp.triangular_solve(lu, sp.lower_triangle, sp.implicit_unit_diagonal, d_pb, d_y)
    sp.triangular_solve(lu, sp.upper_triangle, sp.explicit_diagonal, d_y, d_px)
    sp.permute_vector(L["order"].perm, d_px, d_x, inverse=True)
    assert np.array_equal(U.bits(G.host(d_pb)), U.bits(pb.astype(dtype)))
    assert np.array_equal(U.bits(G.host(d_x)), U.bits(x_true.astype(dtype)))
    # inexact data: the factor of the permuted matrix passes the residual bound, as the host factor of the same ordering does
    rnd = U.dominant_values(L["b_rp"], L["b_ci"], seed=32)
    a_vals[pos] = rnd
    a.values()[:nnz].copy_(G.dev(a_vals.astype(dtype)))
    sp.permute(pinfo, a, L["order"].perm, b)
    sp.ilu0(info, b, lu)
    got = G.host(lu.values())[:nnz]
    assert U.residual_violations(L["b_rp"], L["b_ci"], rnd.astype(dtype), got, dtype) == []
    host = U.host_ilu0(L["b_rp"], L["b_ci"], rnd.astype(dtype), dtype)
    assert U.residual_violations(L["b_rp"], L["b_ci"], rnd.astype(dtype), host, dtype) == []
