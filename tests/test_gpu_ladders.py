"""-m gpu: every row length (SpMV) and every column count (SpMM) the kernels branch on, against float64, under every plan,
value type, layout and pointer alignment -- tests/ladder.py has the generators, the data sets and the checkers, and
tests/test_ladders_cpu.py shows on the host that they contain what they claim and fail what they must.

Each case runs twice: random data against the existing bound of the value type, and integer data whose result must equal
the float64 sum rounded once to the output type, bit for bit.  Outputs are prefilled with NaN (or, inside a
leading-dimension window, a sentinel that must survive in the padding).  Every forced plan is asserted to be the plan
that was built; where the library documents a refusal (SLICED for complex and 16-bit values) the refusal is asserted.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import ladder as L
import spblas_reference_amd as sp
from spblas_reference_amd import _capi
from test_gpu_spmm import PANEL_KERNELS

pytestmark = pytest.mark.gpu

VTS = ["f32", "f64", "c64", "c128", "f16", "bf16"]
CPLX, LOWP = ("c64", "c128"), ("f16", "bf16")
WINDOW_OF = {"f32": "window_f32", "f64": "window_f64", "c64": "window_c64", "c128": "window_c128", "f16": "window_lowp",
             "bf16": "window_lowp"}
CONJ = [(False, False), (True, False), (False, True), (True, True)]
VFREE_ENV = {"SPBLAS_GFX950_PB_VFREE": "2", "SPBLAS_GFX950_PB_VF_ROWS": "500"}
# plan name -> (environment of the inspect call, what sliced_info() must report).  Value-free tiles keep a window of the caller's
# values per bin in LDS: a row longer than that window (ladder.value_free_window_cap: about 40 K entries in fp32, 20 K in
# fp64) cannot be taken, and the full ladder has rows up to 2^17 + 1 -- asked for a value-free plan the library falls back
# to the copying form, which is asserted here.  test_row_length_ladder_spmv_value_free_tiles runs every rung that fits the
# window, the capacity itself included.
SLICED_FORMS = {"sliced_two_byte_rows": ({}, {"row_code_u8": 0}),
                "sliced_one_byte_rows": ({"SPBLAS_GFX950_PB_ENC8": "2"}, {"row_code_u8": 1}),
                "sliced_value_free_asked_falls_back": (VFREE_ENV, {"value_free": 0})}
FORCED = {"vector": _capi.SPMV_VECTOR, "rowblock": _capi.SPMV_ROWBLOCK}


def _data(vt, exact, size_a, size_x, exact_fn):
    """(values, x) as device tensors of the value type and as the float64 / complex128 numbers those tensors hold."""
    cplx = vt in CPLX
    if exact:
        values, x = exact_fn(cplx, vt == "f16")
    else:
        rng = np.random.default_rng(12)
        gen = L.random_complex if cplx else L.random_real
        values, x = gen(rng, size_a), gen(rng, size_x)
    vt_, xt_ = L.cast(vt, values).cuda(), L.cast(vt, x).cuda()
    return vt_, xt_, L.wide(vt_), L.wide(xt_)


def _check(vt, exact, y, ref, absrow, lens, what):
    if exact:
        L.check_exact(vt, y, ref, what)
    else:
        L.check_random(vt, y, ref, absrow, lens, what)


# =============================================================================================== B1: row lengths, SpMV
def _inspect(op, x, y, alg, env, monkeypatch):
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    try:
        return sp.multiply_inspect(op, x, y) if alg is None else sp.multiply_inspect(op, x, y, alg=alg)
    finally:
        for k_ in env:
            monkeypatch.delenv(k_)


@pytest.mark.parametrize("offsets", [np.int32, np.int64], ids=["o32", "o64"])
@pytest.mark.parametrize("vt", VTS)
def test_row_length_ladder_spmv(gpu, vt, offsets, monkeypatch):
    rowptr, colind, shape = L.spmv_ladder()
    m, n = shape
    lens = np.diff(rowptr)
    nnz = int(rowptr[-1])
    th = L.thresholds()
    rp_d, ci_d = torch.from_numpy(rowptr.astype(offsets)).cuda(), torch.from_numpy(colind).cuda()
    dt = L.TORCH_OF[vt]
    ran = set()
    for exact in (False, True):
        vals_d, x_d, values, x = _data(vt, exact, nnz, n, lambda c, h: L.exact_spmv_data(rowptr, colind, n, cplx=c, f16=h))
        a = sp.csr_view(vals_d, rp_d, ci_d, shape, nnz)
        for ca, cx in (CONJ if vt in CPLX else CONJ[:1]):
            ref, absrow = L.spmv_reference(rowptr, colind, values, x, shape, conj_a=ca, conj_x=cx)
            xx = sp.conjugated(x_d) if cx else x_d
            wrap = (lambda t: sp.conjugated(t)) if ca else (lambda t: t)

            def run(name, op, info):
                y = torch.full((m,), float("nan"), dtype=dt, device="cuda")
                if info is None:
                    sp.multiply(op, xx, y)
                else:
                    sp.multiply(info, op, xx, y)
                torch.cuda.synchronize()
                _check(vt, exact, y, ref, absrow, lens, f"{vt} {name} conj={ca, cx} {'exact' if exact else 'random'}")
                ran.add(name)

            y0 = torch.empty(m, dtype=dt, device="cuda")
            run("noplan", wrap(a), None)
            for name, alg in FORCED.items():
                info = _inspect(wrap(a), xx, y0, alg, {}, monkeypatch)
                pi = info.state_.info()
                assert pi["alg"] == alg, f"forced {name} ended up as {pi['alg']}"
                assert pi["max_row_len"] == lens.max()
                if name == "rowblock":      # the window this plan cuts at is one the ladder was built around
                    assert pi["window"] == th[WINDOW_OF[vt]] and pi["n_long_rows"] == int((lens > pi["window"]).sum()), pi
                run(name, wrap(a), info)
            if vt in CPLX or vt in LOWP:     # documented: no SLICED plan for these value types
                with pytest.raises(sp.BackendError) as e:
                    sp.multiply_inspect(wrap(a), xx, y0, alg=_capi.SPMV_SLICED)
                assert e.value.status == _capi.NOT_SUPPORTED
                ran.add("sliced_refused")
            else:
                for name, (env, want) in SLICED_FORMS.items():
                    info = _inspect(a, xx, y0, _capi.SPMV_SLICED, env, monkeypatch)
                    si = info.state_.sliced_info()
                    assert info.state_.info()["alg"] == _capi.SPMV_SLICED, f"forced {name} ended up as {info.state_.info()['alg']}"
                    assert all(si[k_] == v_ for k_, v_ in want.items()), (name, si)
                    run(name, a, info)
            info = _inspect(wrap(a), xx, y0, _capi.SPMV_AUTO, {}, monkeypatch)
            assert info.state_.info()["alg"] in (_capi.SPMV_VECTOR, _capi.SPMV_ROWBLOCK, _capi.SPMV_SLICED)
            run("auto", wrap(a), info)
            a_opt = wrap(sp.matrix_opt(a))
            info = _inspect(a_opt, xx, y0, None, {}, monkeypatch)
            if vt in CPLX or vt in LOWP:
                assert info.state_.info()["alg"] != _capi.SPMV_SLICED
            assert sp.api._find_plan(None, a_opt, a) is info.state_      # the plan travels with the matrix_opt and is found
            run("matrix_opt", a_opt, None)
        if vt in ("f32", "f64"):
            # the same arrays read as CSC: y = A^T x, plan-free -- the scatter kernel and the two-pass form (forced: it is the
            # default from 4 M entries); the ladder's rows are the transposed kernels' segments
            a_csc = sp.csc_view(vals_d, rp_d, ci_d, (n, m), nnz)
            if exact:
                xt = np.random.default_rng(2).integers(-2, 3, m).astype(np.float64)
            else:
                xt = L.random_real(np.random.default_rng(2), m)
            xt_d = L.cast(vt, xt).cuda()
            xt = L.wide(xt_d)
            ref_t = sps.csr_matrix((values, colind, rowptr), shape=shape).T @ xt
            abs_t = sps.csr_matrix((np.abs(values), colind, rowptr), shape=shape).T @ np.abs(xt)
            assert abs_t.max() < 2 ** 24
            col_len = np.bincount(colind, minlength=n)
            for mode in ("0", "1"):
                monkeypatch.setenv("SPBLAS_GFX950_SPMV_T2", mode)
                yt = torch.full((n,), float("nan"), dtype=dt, device="cuda")
                sp.multiply(a_csc, xt_d, yt)
                torch.cuda.synchronize()
                monkeypatch.delenv("SPBLAS_GFX950_SPMV_T2")
                _check(vt, exact, yt, ref_t, abs_t, col_len, f"{vt} transposed, two-pass={mode} {'exact' if exact else 'random'}")
                ran.add(f"transposed_{mode}")
    want = {"noplan", "vector", "rowblock", "auto", "matrix_opt"}
    want |= {"sliced_refused"} if vt in CPLX or vt in LOWP else set(SLICED_FORMS) | {"transposed_0", "transposed_1"}
    assert ran == want, ran ^ want


def _value_free_case(vt, offsets, lengths, env, want_value_free, what, monkeypatch):
    """One ladder through a SLICED plan asked to be value-free: inspected with ZEROS in the value array, the data copied in
    afterwards in place (a value-free plan must read it at the time of the call; the copying form must too), both data sets."""
    rowptr, colind, shape = L.spmv_ladder(lengths=lengths)
    m, n = shape
    lens = np.diff(rowptr)
    nnz = int(rowptr[-1])
    rp_d, ci_d = torch.from_numpy(rowptr.astype(offsets)).cuda(), torch.from_numpy(colind).cuda()
    dt = L.TORCH_OF[vt]
    for exact in (False, True):
        vals_d, x_d, values, x = _data(vt, exact, nnz, n, lambda c, h: L.exact_spmv_data(rowptr, colind, n, cplx=c, f16=h))
        a = sp.csr_view(torch.zeros_like(vals_d), rp_d, ci_d, shape, nnz)
        y = torch.full((m,), float("nan"), dtype=dt, device="cuda")
        info = _inspect(a, x_d, y, _capi.SPMV_SLICED, env, monkeypatch)
        si = info.state_.sliced_info()
        assert info.state_.info()["alg"] == _capi.SPMV_SLICED and info.state_.info()["max_row_len"] == lens.max()
        assert si["value_free"] == want_value_free, (what, si)
        a.values().copy_(vals_d)
        sp.multiply(info, a, x_d, y)
        torch.cuda.synchronize()
        ref, absrow = L.spmv_reference(rowptr, colind, values, x, shape)
        _check(vt, exact, y, ref, absrow, lens, f"{vt} {what} {'exact' if exact else 'random'}")


@pytest.mark.parametrize("offsets", [np.int32, np.int64], ids=["o32", "o64"])
@pytest.mark.parametrize("vt", ["f32", "f64"])
def test_row_length_ladder_spmv_value_free_tiles(gpu, vt, offsets, monkeypatch):
    """Value-free tiles (the plan multiplies with the caller's value array through an LDS window per bin) on every rung that
    fits the window.  One row per bin (test hook): the span of a bin is the length of its row, so the ladder runs up to the
    window's capacity `cap` -- cap - 1 and cap are rungs -- and the same ladder with one row of cap + 1 entries must fall
    back to the copying form (and still be right): the capacity computed from the source is pinned from both sides.
    SPBLAS_GFX950_PB_VARBINS=0 keeps the row map (long rows cut into pieces, empty rows taken out) off, which this
    skewed matrix would otherwise get and which value-free tiles do not take.  Then bins of several rows (500 and 7 asked
    for; the library shrinks them until the widest fits) on the rungs up to the fp32 window + 1."""
    item = 4 if vt == "f32" else 8
    cap = L.value_free_window_cap(item)
    th = L.thresholds()
    lengths = L.value_free_row_lengths(item)
    assert lengths.max() == cap and cap > 8 * th[WINDOW_OF[vt]]
    one_row = {"SPBLAS_GFX950_PB_VFREE": "2", "SPBLAS_GFX950_PB_VF_ROWS": "1", "SPBLAS_GFX950_PB_VARBINS": "0"}
    _value_free_case(vt, offsets, lengths, one_row, 1, f"value-free tiles, one row per bin, rows up to the window ({cap})",
                     monkeypatch)
    _value_free_case(vt, offsets, np.append(lengths, cap + 1), one_row, 0, "value-free asked, one row of cap + 1: copying form",
                     monkeypatch)
    for rows_per_bin in ("500", "7"):
        env = dict(VFREE_ENV, SPBLAS_GFX950_PB_VF_ROWS=rows_per_bin)
        _value_free_case(vt, offsets, L.short_row_lengths(), env, 1, f"value-free tiles, {rows_per_bin} rows per bin", monkeypatch)


# =============================================================================================== B2: column counts, SpMM
def _capi_spmm(vt, plan, a, Bv, Cv, alpha, beta):
    """C = alpha * A B + beta * C through the C ABI (the Python layer has no beta)."""
    m, k = a.shape()
    n = Cv.shape[1]
    hd = sp.api._Handle.current(Cv.device)
    P = sp.api._ptr
    (brs, bcs), (crs, ccs) = sp.api._dense_strides(Bv, k, n), sp.api._dense_strides(Cv, m, n)
    ot = _capi.I64 if a.rowptr().dtype == torch.int64 else _capi.I32
    code = {"f32": _capi.F32, "f64": _capi.F64, "c64": _capi.C32, "c128": _capi.C64, "f16": _capi.F16, "bf16": _capi.BF16}[vt]
    if vt in CPLX:
        ct = sp.api.c_complex64 if vt == "c64" else sp.api.c_complex128
        al, be = ct(alpha), ct(beta)
        rc = _capi.lib().spblas_gfx950_spmm_strided_conj(hd.h, plan, m, k, n, a.size(), ctypes.byref(al), P(a.rowptr()),
                                                         P(a.colind()), P(a.values()), P(Bv), brs, bcs, ctypes.byref(be), P(Cv),
                                                         crs, ccs, ot, code, 0)
    else:
        ct = ctypes.c_double if vt == "f64" else ctypes.c_float
        al, be = ct(alpha), ct(beta)
        rc = _capi.lib().spblas_gfx950_spmm_strided(hd.h, plan, m, k, n, a.size(), ctypes.byref(al), P(a.rowptr()),
                                                    P(a.colind()), P(a.values()), P(Bv), brs, bcs, ctypes.byref(be), P(Cv),
                                                    crs, ccs, ot, code)
    sp.api.check(rc, "spmm through the C ABI")


def _spmm_ladder(vt, layout, ns, shifts, make_info, what):
    """Every n of `ns` x every (B shift, C shift) x both data sets, for one value type and layout.  make_info(a, B, C) ->
    operation_info or None (plan-free).  alpha = 1, beta = 0 through multiply(); on every third n alpha != 1 and beta != 0
    through the C ABI on a C that holds values.  Returns the number of multiplies checked."""
    rowptr, colind, shape = L.spmm_matrix()
    m, k = shape
    lens = np.diff(rowptr)
    nnz = int(rowptr[-1])
    nmax = max(ns)
    dt = L.TORCH_OF[vt]
    rp_d, ci_d = torch.from_numpy(rowptr.astype(np.int32)).cuda(), torch.from_numpy(colind).cuda()
    done = 0
    for exact in (False, True):
        vals_d, B_d, values, B = _data(vt, exact, nnz, (k, nmax),
                                       lambda c, h: L.exact_spmm_data(rowptr, colind, shape, nmax, cplx=c, f16=h))
        a = sp.csr_view(vals_d, rp_d, ci_d, shape, nnz)
        info = make_info(a, B_d[:, :8].contiguous(), torch.empty((m, 8), dtype=dt, device="cuda"))
        ref_all, abs_all = L.spmm_reference(rowptr, colind, values, B, shape)
        alpha, beta = (2.0, -1.0) if exact else (-1.5, 0.5)
        rng = np.random.default_rng(44)
        C0 = rng.integers(-2, 3, (m, nmax)).astype(np.float64) if exact else rng.uniform(-1, 1, (m, nmax))
        C0_d = L.cast(vt, C0).cuda()
        C0 = L.wide(C0_d).real
        for i, n in enumerate(ns):
            scaled = i % 3 == 2
            ref, absr = ref_all[:, :n], abs_all[:, :n]
            if scaled:
                ref, absr = alpha * ref + beta * C0[:, :n], abs(alpha) * absr + abs(beta) * np.abs(C0[:, :n])
            outs, pad_bad = [], torch.zeros((), dtype=torch.bool, device="cuda")
            b_win = {sb: L.dense_window(k, n, layout, sb, dt, "cuda", init=B_d[:, :n])[1] for sb in {s_[0] for s_ in shifts}}
            c_win = {sc: L.dense_window(m, n, layout, sc, dt, "cuda") for sc in {s_[1] for s_ in shifts}}
            for sb, sc in shifts:
                Bv, (c_store, Cv, c_mask) = b_win[sb], c_win[sc]
                c_store.fill_(L.SENTINEL[dt])
                assert Bv.data_ptr() % 16 == (sb * Bv.element_size()) % 16 and Cv.data_ptr() % 16 == (sc * Cv.element_size()) % 16
                if scaled:
                    Cv.copy_(C0_d[:, :n])
                    _capi_spmm(vt, info.state_.plan if info is not None else None, a, Bv, Cv, alpha, beta)
                else:
                    Cv.fill_(float("nan"))
                    if info is None:
                        sp.multiply(a, Bv, Cv)
                    else:
                        sp.multiply(info, a, Bv, Cv)
                outs.append(Cv.contiguous())
                pad_bad |= ~L.padding_untouched_t(c_store, c_mask, dt)
                done += 1
            torch.cuda.synchronize()
            assert not bool(pad_bad), f"{what} n={n}: the padding of a leading-dimension window of C was written"
            got = torch.cat(outs)                      # (shifts * m, n): one transfer and one comparison per n
            reps = len(outs)
            _check(vt, exact, got, np.tile(ref, (reps, 1)), np.tile(absr, (reps, 1)), np.tile(lens, reps),
                   f"{what} n={n} shifts={shifts}{' alpha, beta' if scaled else ''} {'exact' if exact else 'random'}")
    return done


@pytest.mark.parametrize("layout", L.LAYOUTS)
@pytest.mark.parametrize("mode", ["plan_free", "inspected"])
@pytest.mark.parametrize("vt", VTS)
def test_column_count_ladder_spmm(gpu, vt, mode, layout):
    th = L.thresholds()

    def make_info(a, B, C):
        if mode == "plan_free":
            return None
        info = sp.multiply_inspect(a, B, C)
        pi = info.state_.info()
        assert pi["alg"] == _capi.SPMV_ROWBLOCK and pi["window"] == th[WINDOW_OF[vt]] and pi["n_long_rows"] == 3, pi
        assert pi["max_row_len"] > 2 * th["spmm_part_entries"]          # parts > 1 in the long-row kernels
        if vt in ("f32", "f64"):
            assert info.state_.spmm_info()["inspected"] == 1 and info.state_.spmm_info()["long_rows"] == 3
        return info

    done = _spmm_ladder(vt, layout, L.SPMM_NS, L.SHIFTS, make_info, f"{vt} {mode} {layout}")
    assert done == 2 * len(L.SPMM_NS) * len(L.SHIFTS)


PANEL_NS = sorted({n + d for n in L.SPMM_NS if n % 16 == 0 for d in (-1, 0, 1)} & set(L.SPMM_NS))


@pytest.mark.parametrize("kernel", list(PANEL_KERNELS))
def test_column_count_ladder_spmm_panel_kernels(gpu, kernel, monkeypatch):
    """f32, inspected, the band block of the ladder matrix taken by each of the panel kernels (admitted below the performance
    threshold, as test_gpu_spmm.py does): the ladder's multiples of 16 and their neighbours, every layout."""
    for k_, v_ in PANEL_KERNELS[kernel].items():
        monkeypatch.setenv(k_, v_)
    monkeypatch.setenv("SPBLAS_GFX950_SPMM_PANEL_MIN", "64")
    assert {15, 16, 17, 127, 128, 129, 255, 256, 257, 511, 512, 513} <= set(PANEL_NS)

    def make_info(a, B, C):
        info = sp.multiply_inspect(sp.matrix_opt(a), B, C)
        mi = info.state_.spmm_info()
        assert mi["inspected"] == 1 and mi["panel_blocks"] >= (L.BAND_ROWS[1] - L.BAND_ROWS[0]) // 32 - 1, mi
        return info

    for layout in L.LAYOUTS:
        _spmm_ladder("f32", layout, PANEL_NS, [(0, 0), (1, 0), (0, 1), (2, 2)], make_info, f"panel {kernel} {layout}")


@pytest.mark.parametrize("vt", VTS)
def test_spmm_long_row_parts_are_capped(gpu, vt):
    """The long-row kernels cut a row into ceil(len / entries) parts, at most `cap` of them (ladder.spmm_parts_rule): one row of
    more than entries * cap entries reaches the capped branch, where a part is longer than `entries`.  Inspected, row-major,
    n below, at and above the columns per pass and with every tail of the lane width; both data sets."""
    per, cap = L.spmm_parts_rule()
    rowptr, colind, shape = L.spmm_capped_parts_matrix()
    m, k = shape
    lens = np.diff(rowptr)
    nnz = int(rowptr[-1])
    assert lens.max() > per * cap
    dt = L.TORCH_OF[vt]
    ns = [1, 2, 3, 4, 7, 64, 65, 255, 256, 257]
    rp_d, ci_d = torch.from_numpy(rowptr.astype(np.int32)).cuda(), torch.from_numpy(colind).cuda()
    for exact in (False, True):
        vals_d, B_d, values, B = _data(vt, exact, nnz, (k, max(ns)),
                                       lambda c, h: L.exact_spmm_data(rowptr, colind, shape, max(ns), cplx=c, f16=h))
        a = sp.csr_view(vals_d, rp_d, ci_d, shape, nnz)
        ref_all, abs_all = L.spmm_reference(rowptr, colind, values, B, shape)
        info = sp.multiply_inspect(a, B_d[:, :8].contiguous(), torch.empty((m, 8), dtype=dt, device="cuda"))
        pi = info.state_.info()
        assert pi["alg"] == _capi.SPMV_ROWBLOCK and pi["n_long_rows"] == 1 and pi["max_row_len"] == lens.max(), pi
        for n in ns:
            Bv = B_d[:, :n].contiguous()
            C = torch.full((m, n), float("nan"), dtype=dt, device="cuda")
            sp.multiply(info, a, Bv, C)
            torch.cuda.synchronize()
            _check(vt, exact, C, ref_all[:, :n], abs_all[:, :n], lens, f"{vt} capped parts n={n} {'exact' if exact else 'random'}")
