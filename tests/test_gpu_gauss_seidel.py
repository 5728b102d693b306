"""-m gpu tests of gauss_seidel_inspect / gauss_seidel (spblas_gfx950_gs_*, csrc/gauss_seidel.hip) through the Python layer and
the C ABI.  Every test fails on a backend without the feature: the names do not exist there.

The host model (sequential Gauss-Seidel in colour order), the structure check and the generators: tests/gs_util.py, proved on the
host by tests/test_gs_cpu.py.  On the dyadic systems every intermediate is exact, so the device must deliver the model's values
BIT FOR BIT (+-0 alike) whatever its lanes, grid or order of additions; on the dominant systems every row must lie within
2 tol max_r S_r of the float64 model, the bound derived in gs_util's docstring.  Every device array is longer than its contents
and poisoned behind them."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import gpu_util as G
import gs_util as GS
import spblas_reference_amd as sp
from spblas_reference_amd import _capi

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
LANES = (4, 8, 16, 64)
PAD = 5
WILD = 2 ** 30
REFS = {}            # (system key, sweeps, omega, direction) -> the model's x in A's order (float64), computed once


def tdtype(dtype):
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def on_device(rowptr, colind, values, dtype):
    """csr_view over over-long arrays: a wild column and NaN behind nnz."""
    m, nnz = rowptr.size - 1, int(colind.size)
    d_v = G.dev(np.concatenate([np.asarray(values, np.float64), np.full(PAD, np.nan)]).astype(dtype))
    d_ci = G.dev(np.concatenate([colind.astype(np.int32), np.full(PAD, WILD, np.int32)]))
    return sp.csr_view(d_v, G.dev(rowptr.astype(np.int32)), d_ci, (m, m), nnz)


def window(host, dtype, offset=0):
    """`host` as a window of a wider NaN tensor, `offset` elements in."""
    wide = torch.full((host.size + offset + PAD,), float("nan"), dtype=tdtype(dtype), device="cuda")
    wide[offset:offset + host.size].copy_(G.dev(np.asarray(host).astype(dtype)))
    return wide, wide[offset:offset + host.size]


class Form:
    """One system on the device, as A with perm or as B = P A P^T without one, inspected once."""

    def __init__(self, y, dtype, on_b):
        self.y, self.dtype, self.on_b = y, dtype, on_b
        if on_b:
            self.a = on_device(y.b_rowptr, y.b_colind, y.b_values, dtype)
            self.perm, self.b_host, self.x0_host = None, y.pb, y.px0
        else:
            self.a = on_device(y.rowptr, y.colind, y.values, dtype)
            self.perm, self.b_host, self.x0_host = G.dev(y.perm), y.b, y.x0
        self.color_ptr = G.dev(y.color_ptr)
        self.info = sp.gauss_seidel_inspect(self.a, self.color_ptr, self.perm)
        self.b = G.dev(self.b_host.astype(dtype))

    def run(self, sweeps, omega, direction, x0=None):
        """x in A's order on the host; the NaN around x must stay."""
        wide, x = window(self.x0_host if x0 is None else x0, self.dtype, 1)
        sp.gauss_seidel(self.info, self.a, self.b, x, sweeps=sweeps, omega=omega, direction=direction)
        got = G.host(wide)
        assert np.isnan(got[:1]).all() and np.isnan(got[1 + self.y.m:]).all(), "written outside x"
        got = got[1:1 + self.y.m]
        if self.on_b:
            back = np.empty_like(got)
            back[self.y.perm] = got
            return back
        return got


def ref(key, y, sweeps, omega, direction):
    k = (key, sweeps, omega, direction)
    if k not in REFS:
        REFS[k] = GS.reference(y, sweeps, omega, direction, np.float64)
    return REFS[k]


# ---- bit for bit on the dyadic systems ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lanes", LANES)
def test_dyadic_systems_bit_for_bit(gpu, lanes, dtype):
    y = GS.dyadic_system(lanes)
    bad = []
    for on_b in (False, True):
        f = Form(y, dtype, on_b)
        info = f.info.state_.info()
        assert info["lanes_per_row"] == lanes and info["colors"] == y.color_ptr.size - 1
        assert info["max_color_size"] == int(np.diff(y.color_ptr).max())
        assert info["launches_per_forward_sweep"] == int((np.diff(y.color_ptr) > 0).sum())
        for direction in GS.DIRECTIONS:
            for omega in GS.OMEGAS:
                for sweeps in (0, 1, 2):
                    want, _ = ref(("dyadic", lanes), y, sweeps, omega, direction)
                    got = f.run(sweeps, omega, direction)
                    bad += GS.bit_violations(got, want, f"{'B' if on_b else 'A+perm'} {direction} omega {omega} sweeps {sweeps}")
    assert bad == [], bad[:6]


@pytest.mark.parametrize("dtype", DTYPES)
def test_coloured_chain_tells_forward_backward_and_jacobi_apart(gpu, dtype):
    y = GS.colored_chain()
    jac = GS.host_jacobi(y.rowptr, y.colind, y.values, y.b, y.x0)
    for on_b in (False, True):
        f = Form(y, dtype, on_b)
        got = {d: f.run(1, 1.0, d) for d in GS.DIRECTIONS}
        for d in GS.DIRECTIONS:
            assert GS.bit_violations(got[d], ref("chain", y, 1, 1.0, d)[0], d) == []
            assert not np.array_equal(got[d].astype(np.float64), jac)
        assert not np.array_equal(got["forward"], got["backward"])
        for omega in GS.OMEGAS:
            assert GS.bit_violations(f.run(2, omega, "symmetric"), ref("chain", y, 2, omega, "symmetric")[0]) == []


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def _shapes():
    return GS.shape_systems(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("name", ["one_row", "diagonal_one_colour", "empty_first", "empty_middle", "empty_last", "block_minus_1",
                                  "block_exact", "block_plus_1", "forty_colours", "grid_stride"])
def test_shapes_bit_for_bit(gpu, name):
    y = _shapes()[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if name == "grid_stride":
        assert y.color_ptr[1] == cus * 16 * 64 + 1
    bad = []
    for dtype in DTYPES:
        for on_b in ((False,) if name == "grid_stride" else (False, True)):
            f = Form(y, dtype, on_b)
            info = f.info.state_.info()
            assert info["lanes_per_row"] == 4 and info["launches_per_forward_sweep"] == int((np.diff(y.color_ptr) > 0).sum())
            for direction in GS.DIRECTIONS:
                for omega, sweeps in ((1.0, 1), (1.0, 2), (0.5, 1), (1.5, 1)):
                    want, _ = ref(("shape", name, cus), y, sweeps, omega, direction)
                    bad += GS.bit_violations(f.run(sweeps, omega, direction), want, f"{dtype.__name__} {on_b} {direction} {omega}")
    assert bad == [], bad[:6]


# ---- dominant systems: the derived bound -------------------------------------------------------------------------------------
@pytest.mark.parametrize("omega", [1.0, 0.75])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dominant_system_within_the_derived_bound(gpu, dtype, omega):
    y = GS.dominant_system(20000, seed=11)
    want, S = ref("dominant", y, 5, omega, "symmetric")
    for on_b in (False, True):
        got = Form(y, dtype, on_b).run(5, omega, "symmetric")
        assert GS.max_bound_violations(got, want, S, dtype, f"on_b {on_b}") == []


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(GS.multicolor_fixtures()))
def test_multicolour_fixtures_coloured_on_the_device(gpu, name, dtype):
    """multicolor_order -> gauss_seidel on A with perm, and permute -> gauss_seidel on B: the two agree after permute_vector."""
    y = GS.multicolor_system(name)
    m, nnz, td = y.m, y.nnz, tdtype(dtype)
    a = on_device(y.rowptr, y.colind, y.values, dtype)
    order = sp.multicolor_order(a)
    assert np.array_equal(G.host(order.perm), y.perm) and np.array_equal(G.host(order.color_ptr), y.color_ptr)
    pa = sp.csr_view(torch.full((nnz + PAD,), float("nan"), dtype=td, device="cuda"),
                     torch.full((m + 1 + PAD,), WILD, dtype=torch.int32, device="cuda"),
                     torch.full((nnz + PAD,), WILD, dtype=torch.int32, device="cuda"), (m, m), nnz)
    sp.permute(a, order.perm, pa)
    b, x = G.dev(y.b.astype(dtype)), G.dev(y.x0.astype(dtype))
    pb, px, back = (torch.full((m,), float("nan"), dtype=td, device="cuda") for _ in range(3))
    sp.permute_vector(order.perm, b, pb)
    sp.permute_vector(order.perm, x, px)
    on_a = sp.gauss_seidel_inspect(a, order.color_ptr, order.perm)
    on_b = sp.gauss_seidel_inspect(pa, order.color_ptr)
    sp.gauss_seidel(on_a, a, b, x, sweeps=5, direction="symmetric")
    sp.gauss_seidel(on_b, pa, pb, px, sweeps=5, direction="symmetric")
    sp.permute_vector(order.perm, px, back, inverse=True)
    want, S = ref(("multicolor", name), y, 5, 1.0, "symmetric")
    got_a, got_b = G.host(x), G.host(back)
    assert GS.max_bound_violations(got_a, want, S, dtype, "A with perm") == []
    assert GS.max_bound_violations(got_b, want, S, dtype, "permuted B") == []
    assert GS.max_bound_violations(got_a, got_b.astype(np.float64), S, dtype, "A against B") == []


# ---- the contract --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_nan_quiet_rows_windows_repeats_and_edited_values(gpu, dtype):
    y = GS.dyadic_system(8)
    f = Form(y, dtype, False)
    m, nnz = y.m, y.nnz
    vals0, b0 = G.host(f.a.values()).copy(), G.host(f.b).copy()
    # at omega = 1 the old x_r is not read: NaN in the quiet rows comes out as b / d
    x0 = y.x0.copy()
    x0[y.quiet] = np.nan
    want, _ = ref(("dyadic", 8), y, 1, 1.0, "forward")
    assert GS.bit_violations(f.run(1, 1.0, "forward", x0=x0), want, "NaN in quiet rows") == []
    # ... and at omega != 1 it IS read
    assert np.isnan(f.run(1, 0.5, "forward", x0=x0)[y.quiet]).all()
    # x and b as windows of wider tensors at element offsets 0 / 1 / 3: the surroundings stay NaN
    want, _ = ref(("dyadic", 8), y, 2, 1.5, "symmetric")
    for off_x in (0, 1, 3):
        for off_b in (0, 1, 3):
            wide_x, x = window(y.x0, dtype, off_x)
            wide_b, b = window(y.b, dtype, off_b)
            sp.gauss_seidel(f.info, f.a, b, x, sweeps=2, omega=1.5, direction="symmetric")
            hx, hb = G.host(wide_x), G.host(wide_b)
            assert GS.bit_violations(hx[off_x:off_x + m], want, f"offsets {off_x} / {off_b}") == []
            assert np.isnan(hx[:off_x]).all() and np.isnan(hx[off_x + m:]).all()
            assert np.isnan(hb[:off_b]).all() and np.isnan(hb[off_b + m:]).all()
            assert np.array_equal(GS.bits(hb[off_b:off_b + m]), GS.bits(y.b.astype(dtype))), "b changed"
    # b and the values are unchanged (NaN behind nnz included); two calls give the same bits
    assert np.array_equal(GS.bits(G.host(f.a.values())), GS.bits(vals0)) and np.array_equal(GS.bits(G.host(f.b)), GS.bits(b0))
    assert np.array_equal(GS.bits(f.run(2, 0.5, "backward")), GS.bits(f.run(2, 0.5, "backward")))
    # the info holds structure only: values edited between calls are picked up
    new = y.values * np.where(np.arange(nnz) % 3 == 0, -1.0, 1.0)
    f.a.values()[:nnz].copy_(G.dev(new.astype(dtype)))
    edited, _ = GS.host_gauss_seidel(y.rowptr, y.colind, new, y.b, y.x0, y.color_ptr, y.perm, 2, 1.0, "symmetric", np.float64)
    assert GS.bit_violations(f.run(2, 1.0, "symmetric"), edited, "edited values") == []
    # sweeps = 0 launches nothing and leaves x untouched, NaN included
    assert np.array_equal(GS.bits(f.run(0, 1.0, "symmetric", x0=x0)), GS.bits(x0.astype(dtype)))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_every_inspect_violation_is_a_value_error_and_later_calls_still_work(gpu):
    y = GS.dyadic_system(8)
    dtype = np.float32
    cp, perm = G.dev(y.color_ptr), G.dev(y.perm)
    good = on_device(y.rowptr, y.colind, y.values, dtype)
    mk = lambda rp, ci: on_device(rp, ci, np.ones(ci.size), dtype)
    calls = [lambda c=c: sp.gauss_seidel_inspect(good, G.dev(c), perm) for c in GS.bad_color_ptrs(y.color_ptr)]
    calls += [lambda p=p: sp.gauss_seidel_inspect(good, cp, G.dev(p)) for p in GS.bad_perms(y.perm)]
    calls += [lambda rp=rp, ci=ci: sp.gauss_seidel_inspect(mk(rp, ci), cp, perm)
              for rp, ci in GS.bad_structures(y.rowptr, y.colind) + GS.bad_diagonals(y.rowptr, y.colind)]
    calls += [lambda rp=rp, ci=ci: sp.gauss_seidel_inspect(mk(rp, ci), cp, perm) for _, rp, ci in GS.same_colour_pairs(y)]
    calls.append(lambda: sp.gauss_seidel_inspect(good, cp))              # the colouring without its perm: a clash in A's own order
    assert GS.structure_violations(y.rowptr, y.colind, y.color_ptr) != []
    info = sp.operation_info_t()
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        sp.gauss_seidel_inspect(info, good, G.dev(GS.bad_color_ptrs(y.color_ptr)[0]), perm)
    assert info.state_ is None                                          # a refused inspect writes nothing
    f = Form(y, dtype, False)
    assert GS.bit_violations(f.run(2, 1.0, "symmetric"), ref(("dyadic", 8), y, 2, 1.0, "symmetric")[0]) == []
    # an info from another operation, or for other arrays
    b, x = f.b, G.dev(y.x0.astype(dtype))
    with pytest.raises(ValueError):
        sp.gauss_seidel(sp.operation_info_t(), f.a, b, x)
    pa = on_device(y.b_rowptr, y.b_colind, y.b_values, dtype)
    with pytest.raises(ValueError):
        sp.gauss_seidel(sp.ilu0_inspect(pa), pa, b, x)
    with pytest.raises(ValueError):
        sp.gauss_seidel(f.info, on_device(y.rowptr, y.colind, y.values, dtype), b, x)     # the same matrix in other arrays
    with pytest.raises(ValueError):
        sp.gauss_seidel(f.info, f.a, b, b)
    assert np.array_equal(G.host(x), y.x0.astype(dtype))


def test_c_abi_statuses_in_their_documented_order(gpu):
    y = GS.dyadic_system(4)
    f = Form(y, np.float32, False)
    lib, hd, plan = _capi.lib(), f.info.state_.hd.h, f.info.state_.plan
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    x = G.dev(y.x0.astype(np.float32))
    one = ctypes.c_float(1.0)
    w = ctypes.byref(one)
    rp, ci, v, b = p(f.a.rowptr()), p(f.a.colind()), p(f.a.values()), p(f.b)
    m, nnz = y.m, y.nnz

    def sweep(handle=hd, pl=plan, mm=m, nn=nnz, s=1, d=_capi.GS_FORWARD, om=w, bb=b, xx=None, vt=_capi.F32):
        return lib.spblas_gfx950_gs_sweep(handle, pl, mm, nn, s, d, om, rp, ci, v, bb, p(x) if xx is None else xx, vt)

    for vt in (_capi.C32, _capi.C64, _capi.F16, _capi.BF16):
        assert sweep(handle=None, pl=None, vt=vt) == _capi.NOT_SUPPORTED          # before any other check
    assert sweep(handle=None, pl=None) == _capi.INVALID_HANDLE
    assert sweep(pl=None, mm=-1) == _capi.INVALID_POINTER                          # pointers before sizes
    assert sweep(om=None) == _capi.INVALID_POINTER
    assert sweep(bb=None) == _capi.INVALID_POINTER
    assert sweep(mm=-1, d=7) == _capi.INVALID_SIZE                                 # sizes before values
    assert sweep(nn=-1) == _capi.INVALID_SIZE
    assert sweep(d=3, mm=m + 1) == _capi.INVALID_VALUE                             # values before the plan check
    assert sweep(s=-1) == _capi.INVALID_VALUE
    assert sweep(xx=b) == _capi.INVALID_VALUE
    assert sweep(vt=99) == _capi.INVALID_VALUE
    assert sweep(mm=m + 1) == _capi.PLAN_MISMATCH
    assert sweep(nn=nnz - 1) == _capi.PLAN_MISMATCH
    torch.cuda.synchronize()
    assert np.array_equal(G.host(x), y.x0.astype(np.float32)), "a refused call wrote x"
    assert sweep(s=0) == _capi.SUCCESS and sweep(s=2, d=_capi.GS_SYMMETRIC) == _capi.SUCCESS
    torch.cuda.synchronize()
    assert GS.bit_violations(G.host(x), ref(("dyadic", 4), y, 2, 1.0, "symmetric")[0]) == []
    arr = (ctypes.c_int64 * 4)()
    assert lib.spblas_gfx950_gs_info(plan, arr) == _capi.SUCCESS
    assert list(arr) == [y.color_ptr.size - 1, int(np.diff(y.color_ptr).max()), 4, int((np.diff(y.color_ptr) > 0).sum())]
    # the inspect: pointers, sizes, an empty matrix
    new = ctypes.c_void_p()
    cp = p(f.color_ptr)
    create = lambda mm, nn, cols, c: lib.spblas_gfx950_gs_create(hd, ctypes.byref(new), mm, nn, rp, ci, cols, c, None)
    assert create(m, nnz, 5, None) == _capi.INVALID_POINTER
    assert create(-1, nnz, 5, cp) == _capi.INVALID_SIZE and create(m, nnz, -1, cp) == _capi.INVALID_SIZE
    assert create(0, 1, 0, cp) == _capi.INVALID_VALUE and not new.value
    zero = torch.zeros(3, dtype=torch.int32, device="cuda")
    assert create(0, 0, 2, p(zero)) == _capi.SUCCESS                               # m == 0: two empty colours
    assert lib.spblas_gfx950_gs_sweep(hd, new, 0, 0, 3, _capi.GS_SYMMETRIC, w, rp, None, None, None, None, _capi.F32) == \
        _capi.SUCCESS
    assert lib.spblas_gfx950_gs_destroy(hd, new) == _capi.SUCCESS and lib.spblas_gfx950_gs_destroy(hd, None) == _capi.SUCCESS


def test_complex_and_16_bit_values_raise_type_error(gpu):
    y = GS.colored_chain()
    cp = G.dev(y.color_ptr)
    for td in (torch.complex64, torch.complex128, torch.float16, torch.bfloat16):
        a = sp.csr_view(torch.ones(y.nnz, dtype=td, device="cuda"), G.dev(y.b_rowptr), G.dev(y.b_colind), (y.m, y.m), y.nnz)
        with pytest.raises(TypeError):
            sp.gauss_seidel_inspect(a, cp)
        with pytest.raises(TypeError):
            sp.gauss_seidel(sp.operation_info_t(), a, torch.ones(y.m, dtype=td, device="cuda"),
                            torch.ones(y.m, dtype=td, device="cuda"))


# ---- capture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_first_call_of_a_fresh_info_records_into_a_graph(gpu, dtype):
    y = GS.dyadic_system(16)
    f = Form(y, dtype, False)                                      # a fresh info: no sweep has run on it
    eager = Form(y, dtype, False)
    x_g, x_e = G.dev(y.x0.astype(dtype)), G.dev(y.x0.astype(dtype))
    torch.cuda.synchronize()
    raised = []
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        try:
            sp.gauss_seidel_inspect(f.a, f.color_ptr, f.perm)      # inspect-class: refused inside a capture
            raised.append(None)
        except Exception as e:  # noqa: BLE001
            raised.append(e)
        sp.gauss_seidel(f.info, f.a, f.b, x_g, sweeps=1, omega=1.5, direction="symmetric")
    assert isinstance(raised[0], sp.BackendError) and "not supported" in str(raised[0]).lower(), raised
    assert np.array_equal(G.host(x_g), y.x0.astype(dtype)), "the capture itself must not run the sweep"
    for k in range(3):
        g.replay()
        sp.gauss_seidel(eager.info, eager.a, eager.b, x_e, sweeps=1, omega=1.5, direction="symmetric")
    torch.cuda.synchronize()
    assert np.array_equal(GS.bits(G.host(x_g)), GS.bits(G.host(x_e)))
    assert np.isfinite(G.host(x_g)).all()


# ---- leaks ---------------------------------------------------------------------------------------------------------------------
def test_inspect_sweep_drop_cycles_do_not_leak_device_memory(gpu):
    y = GS.dominant_system(20000, seed=11)
    a = on_device(y.rowptr, y.colind, y.values, np.float32)
    cp, perm = G.dev(y.color_ptr), G.dev(y.perm)
    b, x = G.dev(y.b.astype(np.float32)), G.dev(y.x0.astype(np.float32))

    def cycle():
        info = sp.gauss_seidel_inspect(a, cp, perm)
        sp.gauss_seidel(info, a, b, x, direction="symmetric")
        del info

    for _ in range(8):      # warm-up: the stream-ordered pool reaches its size
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
    # one plan keeps 2 m int32 = 160 KB: 200 leaked plans would be 32 MB
    assert lost < 8 * 2 ** 20, f"free device memory fell by {lost / 2**20:.1f} MiB over 200 cycles"
