"""-m gpu: the ladder of the plan-free transposed SpMV, y = alpha A^T x + beta y on an operand that was never inspected
(tests/ladder_t2.py has the families, the restated geometry and the host model; tests/test_ladders_t2_cpu.py proves on the host
that the families hold their rungs and that the checker bites).

Every case goes through the C ABI (spblas_gfx950_spmv, OP_T) with the two-pass form forced for its size
(SPBLAS_GFX950_SPMV_T2=1, the family's slice width and segment length through _T2_W / _T2_SEG) and FIRST asserts that
spblas_gfx950_spmv_t_last reports the restated geometry -- path, W, S, tiles, segment length, the number of work items --, so
a hook that was ignored or a silent fall-back to the scatter kernel fails the case instead of passing it.  Then y: the integer
and the row-probe set bit for bit (every partial sum is exact, the order of the atomic additions cannot matter), the random
set under the existing parity bound with row_len = entries per column + 1.  The same cases with SPBLAS_GFX950_SPMV_T2=0 (the
scatter kernel) must give the same bits.  y is longer than n; what lies behind n must survive.  No case skips.
"""
import ctypes

import numpy as np
import pytest
import torch

import ladder as L
import ladder_t2 as LT
import spblas_reference_amd as sp
from spblas_reference_amd import _capi

pytestmark = pytest.mark.gpu

VTS = ["f32", "f64"]
OFFSETS = {"o32": np.int32, "o64": np.int64}
SLACK, SENTINEL = 64, -7.25
F = LT.families()

GROUPS = {
    "tiles": [n for n in F if n.startswith("tiles_")],
    "row_starts": [n for n in F if n.startswith(("starts_", "row", "one_row", "last_of_"))],
    "empty_rows_few": [n for n in F if n.startswith(("empty_1_", "empty_2_", "empty_1023_"))],
    "empty_rows_many": [n for n in F if n.startswith(("empty_1024_", "empty_1025_", "empty_5000_"))],
    "slices_W64": [n for n in F if n.startswith("slices_W64_")],
    "slices_wider": [n for n in F if n.startswith("slices_") and not n.startswith("slices_W64_")],
    "segments": [n for n in F if n.startswith(("shares_", "all_1024", "worst_case", "cut_slice"))],
    "item_lengths_uncut": [n for n in F if n.startswith(("item_lengths_uncut", "segment_in_one"))],
    "item_lengths_last_segment": [n for n in F if n.startswith("item_lengths_last_segment")],
    "scan_edges": [n for n in F if n.startswith("scan_")],
}
assert sorted(sum(GROUPS.values(), [])) == sorted(n for n in F if not n.startswith(("widest_", "state_")))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


_ITEMS = {}


def _expected(ff, vt, mode):
    """What spmv_t_last must report for the family under SPBLAS_GFX950_SPMV_T2=mode (restated on the host)."""
    key = (ff.name, vt, mode)
    if key not in _ITEMS:
        g = LT.geometry(vt, ff.shape, ff.nnz, ff.env(mode), _cus())
        g["n_items"] = LT.derived(ff, g)["n_items"] if g["path"] == "two_pass" else -1
        if mode == "0":
            assert (g["path"], g["why"]) == ("scatter", "not_wanted")
        _ITEMS[key] = g
    return _ITEMS[key]


class Dev:
    """One data set of a family on the device (values and x rounded to the value type once; the references are float64)."""

    def __init__(self, ff, kind, vt, offsets):
        self.ff, self.kind, self.vt, self.dt = ff, kind, vt, L.TORCH_OF[vt]
        self.m, self.n = ff.shape
        values, x, _, _, self.cnt = LT.host_data(ff, kind)
        self.rp = torch.from_numpy(ff.rowptr.astype(OFFSETS[offsets])).cuda()
        self.ci = torch.from_numpy(ff.colind).cuda()
        self.vals, self.x = L.cast(vt, values.copy()).cuda(), L.cast(vt, x.copy()).cuda()      # (the shared arrays are read-only)
        self.y0 = LT.y_start(self.n)
        self.hd = sp.api._Handle.current(self.rp.device)

    def new_y(self, beta):
        yb = torch.full((self.n + SLACK,), SENTINEL, dtype=self.dt, device="cuda")
        if beta == 0.0:
            yb[:self.n] = float("nan")
        else:
            yb[:self.n] = L.cast(self.vt, self.y0).cuda()
        return yb

    def spmv(self, alpha, beta, yb):
        ct = sp.api._VT[self.dt][1]
        a_, b_ = ct(alpha), ct(beta)
        hd = sp.api._Handle.current(yb.device)
        sp.api.check(_capi.lib().spblas_gfx950_spmv(hd.h, None, _capi.OP_T, self.m, self.n, self.ff.nnz, ctypes.byref(a_),
                                                    sp.api._ptr(self.rp), sp.api._ptr(self.ci), sp.api._ptr(self.vals),
                                                    sp.api._ptr(self.x), ctypes.byref(b_), sp.api._ptr(yb),
                                                    sp.api._OT[self.rp.dtype], sp.api._VT[self.dt][0]), "spmv")
        return hd

    def check(self, yb, alpha, beta, what):
        torch.cuda.synchronize()
        what = f"{self.ff.name} {self.vt} {self.kind} alpha={alpha} beta={beta} {what}"
        assert bool((yb[self.n:] == SENTINEL).all()), f"{what}: the multiply wrote behind y"
        ref, mag = LT.reference(self.ff, self.kind, alpha, beta, self.y0)
        if self.kind == "random":
            L.check_random(self.vt, yb[:self.n], ref, mag, self.cnt + 1, what)
        else:
            if self.kind == "probe" and (alpha, beta) == (1.0, 0.0):
                assert np.array_equal(ref, LT.row_map(self.ff))
            L.check_exact(self.vt, yb[:self.n], ref, what)


def _run(dev, alpha, beta, mode, monkeypatch, want=None):
    """One call under the family's hooks; the readback is asserted BEFORE y is looked at."""
    env = dev.ff.env(mode)
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    try:
        yb = dev.new_y(beta)
        hd = dev.spmv(alpha, beta, yb)
        got = hd.spmv_t_last()
    finally:
        for k_ in env:
            monkeypatch.delenv(k_)
    want = _expected(dev.ff, dev.vt, mode) if want is None else want
    assert got == want, (dev.ff.name, dev.vt, mode, {k_: (got[k_], want[k_]) for k_ in want if got[k_] != want[k_]})
    dev.check(yb, alpha, beta, f"T2={mode}")
    return got


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_t2_ladder(gpu, vt, offsets, group, monkeypatch):
    """Every family of the group: three data sets x four (alpha, beta) x the two-pass form and the scatter kernel."""
    ran = 0
    for name in GROUPS[group]:
        for kind, ff in LT.cases(F[name]):
            dev = Dev(ff, kind, vt, offsets)
            want = _expected(ff, vt, "1")
            if name == "slices_1025_falls_back":
                assert (want["path"], want["why"], want["S"]) == ("scatter", "does_not_fit", 1025)
            else:
                assert want["path"] == "two_pass", (name, want)
            if ff.W is not None:        # the hook was taken -- or, wider than the LDS holds in fp64, reported as ignored
                assert (want["W"] == ff.W and not want["w_hook_ignored"]) or (ff.W > LT.wcap(vt) and want["w_hook_ignored"] == 1)
            for alpha, beta in LT.ALPHA_BETA:
                for mode in ("1", "0"):
                    _run(dev, alpha, beta, mode, monkeypatch)
                    ran += 1
    assert ran == len(GROUPS[group]) * 3 * 4 * 2


@pytest.mark.parametrize("vt", VTS)
def test_t2_widest_default_geometry(gpu, vt, monkeypatch):
    """No _T2_W hook: n = SMAX slices of the widest slice the LDS holds (y of 160 MB), entries on the slice edges only -- exactly
    SMAX slices; one more column and the call must fall back to the scatter kernel (and still be right).  Compared on the
    device: the integer set, beta = 0 over NaN and beta = 0.5."""
    for name, path in ((f"widest_{vt}", "two_pass"), (f"widest_{vt}_plus_1", "scatter")):
        ff = F[name]
        dev = Dev(ff, "ints", vt, "o32")
        want = _expected(ff, vt, "1")
        assert want["path"] == path and ff.W is None
        if path == "two_pass":
            assert (want["W"], want["S"]) == (LT.wide_w(vt), LT.constants()["SMAX"])
        else:
            assert want["why"] == "does_not_fit"
        y0_d = L.cast(vt, dev.y0).cuda()
        for alpha, beta in ((1.0, 0.0), (-2.0, 0.5)):
            monkeypatch.setenv(LT.PRE, "1")
            try:
                yb = torch.full((dev.n + SLACK,), SENTINEL, dtype=dev.dt, device="cuda")
                yb[:dev.n] = float("nan") if beta == 0.0 else y0_d
                got = dev.spmv(alpha, beta, yb).spmv_t_last()
            finally:
                monkeypatch.delenv(LT.PRE)
            assert got == want, (name, got, want)
            ref, _ = LT.reference(ff, "ints", alpha, beta, dev.y0)
            ref_d = L.cast(vt, ref).cuda()
            torch.cuda.synchronize()
            assert bool((yb[dev.n:] == SENTINEL).all()), f"{name}: the multiply wrote behind y"
            bad = (yb[:dev.n] != ref_d).nonzero()[:5].flatten().tolist()       # (NaN != anything; +0 == -0)
            assert not bad, (name, alpha, beta, bad, yb[bad].tolist(), ref_d[bad].tolist())
            del yb, ref_d


@pytest.mark.parametrize("vt", VTS)
def test_t2_ladder_through_the_host_layer(gpu, vt, monkeypatch):
    """The tile and slice families once through multiply(csc_view ...) and multiply(scaled(alpha, transposed(a)) ...): the same
    readback, the integer set exact."""
    ran = 0
    for name in GROUPS["tiles"] + GROUPS["slices_W64"] + GROUPS["slices_wider"]:
        ff = F[name]
        dev = Dev(ff, "ints", vt, "o32")
        a = sp.csr_view(dev.vals, dev.rp, dev.ci, ff.shape, ff.nnz)
        a_csc = sp.csc_view(dev.vals, dev.rp, dev.ci, (dev.n, dev.m), ff.nnz)
        want = _expected(ff, vt, "1")
        for alpha, op in ((1.0, a_csc), (-2.0, sp.scaled(-2.0, sp.transposed(a)))):
            env = ff.env("1")
            for k_, v_ in env.items():
                monkeypatch.setenv(k_, v_)
            try:
                y = torch.full((dev.n,), float("nan"), dtype=dev.dt, device="cuda")
                sp.multiply(op, dev.x, y)
                got = sp.api._Handle.current(y.device).spmv_t_last()
            finally:
                for k_ in env:
                    monkeypatch.delenv(k_)
            assert got == want, (name, {k_: (got[k_], want[k_]) for k_ in want if got[k_] != want[k_]})
            L.check_exact(vt, y, LT.reference(ff, "ints", alpha, 0.0, dev.y0)[0], f"{name} host layer alpha={alpha}")
            ran += 1
    assert ran == 2 * len(GROUPS["tiles"] + GROUPS["slices_W64"] + GROUPS["slices_wider"])


@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_t2_state_between_calls(gpu, vt, offsets, monkeypatch):
    """One handle, whose scratch is reused: 17 tiles x 1 024 slices, then 1 tile x 1 slice, then the first again.  Stale
    counts, items or a stale item count would show: all three exact."""
    big, small = F["state_17x1024"], F["state_1x1"]
    wb, ws = _expected(big, vt, "1"), _expected(small, vt, "1")
    assert (wb["ntile"], wb["S"]) == (17, 1024) and (ws["ntile"], ws["S"]) == (1, 1) and wb["n_items"] > 2 * 1024
    devs = {ff.name: Dev(ff, "ints", vt, offsets) for ff in (big, small)}
    handles = set()
    for ff in (big, small, big):
        for alpha, beta in ((1.0, 0.0), (-2.0, 0.5)):
            _run(devs[ff.name], alpha, beta, "1", monkeypatch)
            handles.add(devs[ff.name].hd.h.value)
    assert len(handles) == 1


@pytest.mark.parametrize("vt", VTS)
def test_t2_inside_a_stream_capture_keeps_the_scatter_kernel(gpu, vt, monkeypatch):
    """Recorded into a graph the call must not touch the handle's scratch: the readback says scatter, capturing; the replayed
    result is exact."""
    ff = F["shares_seg64"]
    dev = Dev(ff, "ints", vt, "o32")
    want = dict(_expected(ff, vt, "1"), path="scatter", why="capturing", n_items=-1)
    env = ff.env("1")
    _run(dev, 1.0, 0.0, "1", monkeypatch)        # (once outside the capture: the two-pass form, as restated)
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    try:
        yb = dev.new_y(0.0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            hd = dev.spmv(1.0, 0.0, yb)
            got = hd.spmv_t_last()
        assert got == want, {k_: (got[k_], want[k_]) for k_ in want if got[k_] != want[k_]}
        g.replay()
        dev.check(yb, 1.0, 0.0, "captured")
    finally:
        for k_ in env:
            monkeypatch.delenv(k_, raising=False)
