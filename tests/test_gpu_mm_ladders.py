"""-m gpu: the block ladder of the fp32 panel / band path of csrc/spmm.hip (tests/ladder_mm.py has the matrices, the restated
probe and the reference; tests/test_ladders_mm_cpu.py shows on the host that they hold what they claim).

Every family runs under five kernel selections (the band entry loop with 8, 4 and 16 waves, the band path with every fitting
block on the matrix cores, the tile kernel), with int32 and int64 offsets.  A run first asserts that what the inspect decided
(spmm_blocks(): counts, the kind of every block, window and tiles of the qualifying ones) IS the restated probe, then looks
at C: integer data must give the fp64 result bit for bit for three (alpha, beta) through the C ABI, for n in {1, 3, 4, 128,
130, 257}, with B and C shifted by 0 and by 1 element and C inside a wider tensor whose frame must stay untouched; random
data must meet the project's bound (ladder.check_random).  One plan serves every n of a run.  The three families of 65 K rows
take the random data at n = 3 and 130 only (a host-side check of 17 M elements per call otherwise).
"""
import ctypes

import numpy as np
import pytest
import torch

import ladder as L
import ladder_mm as M
import spblas_reference_amd as sp
from spblas_reference_amd import _capi

pytestmark = pytest.mark.gpu
KNOBS = [M.E + s for s in ("PANEL_MIN", "BAND", "BAND_CH", "BAND_WAVES", "BAND_DENSE", "NO_PANEL", "DBG")]
SHIFTS = ((0, 0), (1, 1))
LAYOUT = "right_ld+4"


def _inspect(a, B, C, env, monkeypatch):
    """multiply_inspect under exactly `env` (spmm_inspect_typed reads its knobs at every inspect, the multiplies read none)."""
    for k_ in KNOBS:
        monkeypatch.delenv(k_, raising=False)
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    try:
        return sp.multiply_inspect(a, B, C)
    finally:
        for k_ in env:
            monkeypatch.delenv(k_)


def _assert_blocks(f, info, env):
    """What the inspect decided is what the restated probe decides: before any value is looked at."""
    kn = M.knobs(env)
    kind, nt, tiles, win, panel_nnz = M.probe_family(f, env)
    lens = np.diff(f.rowptr)
    pi = info.state_.info()
    assert pi["window"] == M.constants()["WINDOW"] and pi["n_long_rows"] == int((lens > pi["window"]).sum()), pi
    got = info.state_.spmm_blocks()
    want = {"inspected": 1, "nblk": len(kind), "npanel": int((kind > 0).sum()), "ndense": int((kind == 2).sum()),
            "panel_nnz": panel_nnz, "band": kn["band"], "band_ch": kn["band_ch"], "band_waves": kn["band_waves"],
            "band_dense_pm": kn["dense_pm"], "min_per_tile": kn["min_per_tile"]}
    assert {k_: got[k_] for k_ in want} == want, f.name
    bad = np.flatnonzero(got["kind"] != kind)
    assert not len(bad), f"{f.name}: blocks {bad[:8].tolist()} are of kind {got['kind'][bad[:8]].tolist()}, the probe says {kind[bad[:8]].tolist()}"
    assert np.array_equal(got["tiles"][:, 0], nt), f"{f.name}: tile counts differ at {np.flatnonzero(got['tiles'][:, 0] != nt)[:8].tolist()}"
    for b in np.flatnonzero(kind > 0):
        assert tuple(got["win"][b]) == tuple(win[b]), f"{f.name} block {b}: window {got['win'][b]}, the probe says {win[b]}"
        assert np.array_equal(got["tiles"][b, 1:1 + nt[b]], tiles[b]), f"{f.name} block {b}: tiles {got['tiles'][b]}"
    mi = info.state_.spmm_info()
    assert mi == {"inspected": 1, "panel_blocks": want["npanel"], "panel_nnz": panel_nnz, "long_rows": pi["n_long_rows"]}
    return kind


def _spmm_c_abi(plan, a, Bv, Cv, alpha, beta):
    """C = alpha A B + beta C through spblas_gfx950_spmm itself (row-major operands with leading dimensions)."""
    m, k = a.shape()
    n = Cv.shape[1]
    hd = sp.api._Handle.current(Cv.device)
    P = sp.api._ptr
    al, be = ctypes.c_float(alpha), ctypes.c_float(beta)
    ot = _capi.I64 if a.rowptr().dtype == torch.int64 else _capi.I32
    ldb, ldc = (Bv.stride(0) if k > 1 else n), (Cv.stride(0) if m > 1 else n)
    sp.api.check(_capi.lib().spblas_gfx950_spmm(hd.h, plan, m, k, n, a.size(), ctypes.byref(al), P(a.rowptr()), P(a.colind()),
                                                 P(a.values()), P(Bv), ldb, ctypes.byref(be), P(Cv), ldc, ot, _capi.F32),
                 "spblas_gfx950_spmm")


_REF = {}


def _reference(f, exact):
    """The family's data and its fp64 product for all NMAX columns, computed once and shared by every selection: exact ->
    device tensors (values, B, C0 as fp32; A B and C0 as fp64), random -> (values, B) on the device, A B and sum |a||b| on the host."""
    key = (f.name, f.k, f.nnz, exact)
    if key not in _REF:
        if len(_REF) >= 64:          # (a group's families, both data sets: kept while the selections of the group run)
            _REF.clear()
        values, B, C0 = M.exact_data(f) if exact else M.random_data(f)
        v32, B32, C32 = (torch.from_numpy(np.asarray(x)).float() for x in (values, B, C0))
        AB, absr = M.reference(f, v32.double().numpy(), B32.double().numpy())
        if exact:
            _REF[key] = (v32.cuda(), B32.cuda(), C32.cuda(), torch.from_numpy(AB).cuda(), C32.double().cuda())
        else:
            _REF[key] = (v32.cuda(), B32.cuda(), None, AB, absr)
    return _REF[key]


def _run(f, env, offsets, monkeypatch, ns=M.NS, shifts=SHIFTS):
    rp, ci = f.arrays(offsets)
    rp_d, ci_d = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()
    lens = np.diff(f.rowptr)
    m, k = f.shape
    ft = torch.float32
    done = 0
    # ---- integer data: bit for bit, three (alpha, beta), through the C ABI
    v_d, B_d, C0_d, AB_d, C0_d64 = _reference(f, True)
    a = sp.csr_view(v_d, rp_d, ci_d, f.shape, f.nnz)
    info = _inspect(a, B_d[:, :8].contiguous(), torch.empty((m, 8), device="cuda"), env, monkeypatch)
    _assert_blocks(f, info, env)
    for n in ns:
        outs = []
        for sb, sc in shifts:
            Bv = L.dense_window(k, n, LAYOUT, sb, ft, "cuda", init=B_d[:, :n])[1]
            for alpha, beta in M.ALPHA_BETA:
                c_store, Cv, c_mask = L.dense_window(m, n, LAYOUT, sc, ft, "cuda")
                assert Bv.data_ptr() % 16 == 4 * sb and Cv.data_ptr() % 16 == 4 * sc
                if beta == 0.0:
                    Cv.fill_(float("nan"))
                else:
                    Cv.copy_(C0_d[:, :n])
                _spmm_c_abi(info.state_.plan, a, Bv, Cv, alpha, beta)
                done += 1
                want = (alpha * AB_d[:, :n] + beta * C0_d64[:, :n]).float()
                outs.append((f"n={n} shifts=({sb}, {sc}) alpha={alpha} beta={beta}", Cv, want, L.padding_untouched_t(c_store, c_mask, ft)))
        ok = torch.stack([torch.stack([(c == w).all(), pad]) for _, c, w, pad in outs]).cpu().numpy()
        for (what, c, w, _), (same, pad) in zip(outs, ok):
            assert pad, f"{f.name} {what}: the frame around C was written"
            if not same:
                rows = (c != w).any(dim=1).nonzero().flatten()
                raise AssertionError(f"{f.name} {what}: {len(rows)} rows differ from the exact result, first {rows[:8].tolist()} "
                                     f"(blocks {sorted(set((rows // 32).tolist()))[:8]}): got {c[rows[0]][:6].tolist()}, "
                                     f"want {w[rows[0]][:6].tolist()}")
    # ---- random data: the project's bound, through the Python layer
    v_d, B_d, _, AB, absr = _reference(f, False)
    a = sp.csr_view(v_d, rp_d, ci_d, f.shape, f.nnz)
    info = _inspect(a, B_d[:, :8].contiguous(), torch.empty((m, 8), device="cuda"), env, monkeypatch)
    for n in (ns if m <= 10000 else [n_ for n_ in ns if n_ in (3, 130)]):
        for sb, sc in shifts:
            Bv = L.dense_window(k, n, LAYOUT, sb, ft, "cuda", init=B_d[:, :n])[1]
            c_store, Cv, c_mask = L.dense_window(m, n, LAYOUT, sc, ft, "cuda")
            Cv.fill_(float("nan"))
            sp.multiply(info, a, Bv, Cv)
            done += 1
            assert L.padding_untouched(c_store, c_mask, ft), f"{f.name} n={n}: the frame around C was written"
            L.check_random("f32", Cv.contiguous(), AB[:, :n], absr[:, :n], lens, f"{f.name} n={n} shifts=({sb}, {sc}) random")
    return done


CASES = [(g, s) for g in M.GROUPS for s in M.SELECTIONS]


@pytest.mark.parametrize("offsets", [np.int32, np.int64], ids=["o32", "o64"])
@pytest.mark.parametrize("group,selection", CASES, ids=[f"{g}-{s}" for g, s in CASES])
def test_block_ladder(gpu, group, selection, offsets, monkeypatch):
    fams = M.group(group, selection)
    assert fams
    done = sum(_run(f, M.env_of(f, selection), offsets, monkeypatch) for f in fams)
    small = sum(f.m <= 10000 for f in fams)
    assert done == len(SHIFTS) * (len(fams) * len(M.NS) * len(M.ALPHA_BETA) + small * len(M.NS) + (len(fams) - small) * 2)


@pytest.mark.parametrize("selection", list(M.SELECTIONS))
def test_the_largest_chunk_fits_the_lds_under_every_selection(gpu, selection, monkeypatch):
    """BAND_CH = 312 beside 16 waves' hand-over buffers, and beside the matrix-core kernel's A tile, is more LDS than a
    workgroup can have: such launches were refused (HIP error from the multiply).  The inspect now stages 304 rows beside 16
    waves and the matrix-core kernel takes windows of at most 248 rows."""
    f = M.fam_row_shapes("w244")
    env = M.env_of(f, selection)
    assert env[M.E + "BAND_CH"] == "312"
    kn = M.knobs(env)
    assert kn["band_ch"] == (304 if selection == "band_16_waves" else 312)
    assert _run(f, env, np.int32, monkeypatch, ns=(128, 130)) == 2 * len(SHIFTS) * (len(M.ALPHA_BETA) + 1)


@pytest.mark.parametrize("selection", list(M.SELECTIONS))
def test_one_infinity_in_b_reaches_the_one_row_that_references_it(gpu, selection, monkeypatch):
    """B[INF_ROW, INF_COL] = inf; one row of the matrix references that row of B.  Every other row stays finite and exact --
    the 31 rows that share its block, and the block whose window ends right below INF_ROW: for the matrix-core kernel the row
    lies in the zero-padded tail of that block's staged window."""
    f = M.fam_inf()
    env = M.env_of(f, selection)
    values, B, C0 = M.exact_data(f)
    B[M.INF_ROW, M.INF_COL] = np.inf
    rp_d, ci_d = torch.from_numpy(f.arrays()[0]).cuda(), torch.from_numpy(f.colind).cuda()
    v_d, B_d = torch.from_numpy(values).float().cuda(), torch.from_numpy(B).float().cuda()
    a = sp.csr_view(v_d, rp_d, ci_d, f.shape, f.nnz)
    info = _inspect(a, B_d[:, :8].contiguous(), torch.empty((f.m, 8), device="cuda"), env, monkeypatch)
    kind = _assert_blocks(f, info, env)
    assert list(kind) == ([2, 0, 2, 0] if selection == "band_mfma" else [1, 0, 1, 0])
    for n in (4, 128, 130):
        ref, _ = M.reference(f, values, B[:, :n])
        bad = ~np.isfinite(ref)
        assert bad.sum() == 1 and bad[64 + 5, M.INF_COL]
        for sb, sc in SHIFTS:
            Bv = L.dense_window(f.k, n, LAYOUT, sb, torch.float32, "cuda", init=B_d[:, :n])[1]
            c_store, Cv, c_mask = L.dense_window(f.m, n, LAYOUT, sc, torch.float32, "cuda")
            Cv.fill_(float("nan"))
            _spmm_c_abi(info.state_.plan, a, Bv, Cv, 1.0, 0.0)
            got = Cv.cpu().numpy()
            assert np.isfinite(got[~bad]).all(), f"n={n}: rows {np.flatnonzero(~np.isfinite(got).all(axis=1) & ~bad.any(axis=1)).tolist()} are not finite"
            assert np.array_equal(got, ref.astype(np.float32)), f"n={n} shifts=({sb}, {sc})"
            assert L.padding_untouched(c_store, c_mask, torch.float32)


@pytest.mark.parametrize("selection", list(M.SELECTIONS))
def test_block_ladder_inside_a_stream_capture(gpu, selection, monkeypatch):
    """Dense, entry-loop and row-group blocks interleaved, recorded into a graph after a warm call and replayed on new B."""
    f = M.fam_lists(9, mix=True)
    env = M.env_of(f, selection)
    v_d, B_d, C0_d, AB_d, C0_d64 = _reference(f, True)
    a = sp.csr_view(v_d, torch.from_numpy(f.arrays()[0]).cuda(), torch.from_numpy(f.colind).cuda(), f.shape, f.nnz)
    n = 130
    Bv = B_d[:, :n].contiguous()
    Cv = torch.full((f.m, n), float("nan"), device="cuda")
    info = _inspect(a, Bv, Cv, env, monkeypatch)
    _assert_blocks(f, info, env)
    sp.multiply(info, a, Bv, Cv)                      # the warm call
    torch.cuda.synchronize()
    assert torch.equal(Cv, AB_d[:, :n].float())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sp.multiply(info, a, Bv, Cv)
        with pytest.raises(sp.BackendError) as e:     # the read-back synchronises: refused while the stream records
            info.state_.spmm_blocks()
        assert e.value.status == _capi.NOT_SUPPORTED
    Bv.copy_(-B_d[:, 100:100 + n])
    Cv.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(Cv, -AB_d[:, 100:100 + n].float())


def test_spmm_blocks_statuses_and_plans_the_probe_did_not_run_on(gpu, monkeypatch):
    lib = _capi.lib()
    f = M.fam_lists(3)
    v_d, B_d, _, _, _ = _reference(f, True)
    rp_d, ci_d = torch.from_numpy(f.arrays()[0]).cuda(), torch.from_numpy(f.colind).cuda()
    a = sp.csr_view(v_d, rp_d, ci_d, f.shape, f.nnz)
    Bv, Cv = B_d[:, :8].contiguous(), torch.empty((f.m, 8), device="cuda")
    info = _inspect(a, Bv, Cv, f.env, monkeypatch)
    hd = sp.api._Handle.current(Cv.device)
    counts = (ctypes.c_int64 * 10)()
    assert lib.spblas_gfx950_spmm_plan_blocks(None, info.state_.plan, counts, None, None, None) == _capi.INVALID_HANDLE
    assert lib.spblas_gfx950_spmm_plan_blocks(hd.h, None, counts, None, None, None) == _capi.INVALID_POINTER
    assert lib.spblas_gfx950_spmm_plan_blocks(hd.h, info.state_.plan, None, None, None, None) == _capi.INVALID_POINTER
    assert lib.spblas_gfx950_spmm_plan_blocks(hd.h, info.state_.plan, counts, None, None, None) == 0 and counts[1] == 6
    zero = dict.fromkeys(("inspected", "nblk", "npanel", "ndense", "panel_nnz", "band", "band_ch", "band_waves", "band_dense_pm",
                          "min_per_tile"), 0)

    def counts_of(info_):
        got = info_.state_.spmm_blocks()
        assert all(got[k_].size == 0 for k_ in ("kind", "win", "tiles"))
        return {k_: got[k_] for k_ in zero}

    assert counts_of(_inspect(a, Bv, Cv, dict(f.env, **{M.E + "NO_PANEL": "1"}), monkeypatch)) == zero
    a64 = sp.csr_view(v_d.double(), rp_d, ci_d, f.shape, f.nnz)
    assert counts_of(_inspect(a64, Bv.double(), Cv.double(), f.env, monkeypatch)) == zero
    few = sp.csr_view(v_d[:255].clone(), torch.clamp(rp_d, max=255), ci_d[:255].clone(), f.shape, 255)
    assert counts_of(_inspect(few, Bv, Cv, f.env, monkeypatch)) == zero
