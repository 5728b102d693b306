"""-m gpu: the block-to-thread mapping of the SLICED expand (csrc/expand_map.hpp) on the device.  A wavefront takes L = 2 * 64 /
lanes-per-block consecutive blocks per iteration (16 for fp32, 32 for fp64) and the workgroup 16 * L, so the families here hold
slices of 1, 7, 8, 9, L - 1, L, L + 1, 16 L - 1, 16 L, 16 L + 1 and 2 * 16 L + 1 blocks, and of 127 / 128 / 129 (fp32) or
255 / 256 / 257 (fp64) blocks -- a workgroup pass of the kernel of before --, with empty slices between them.  Inside a slice
the runs have 1 ... 5, 28, 29 ... 36 and 60 ... 68 entries, rotated from slice to slice, so that a slice's first block and the
block after every short run start on each of the eight 16-byte phases of a 128-byte line of the compact stream (asserted);
the last run of the last slice is a whole number of blocks, so its last block ends on the last entry of s_val / s_col.

Three families per value type: `items` (one slice above 3 x the mean: the expand takes its work list, the big slices cut in
parts), `shares` (the same slices plus even ones: equal shares of some hundred blocks, whose boundaries fall inside slices and
which span several slices) and `small_shares` (64-column slices: shares of a few blocks, shorter than one wavefront's L).
As in tests/test_gpu_sliced_ladders.py, whose device harness this file imports, every case asserts alg == SLICED and info() /
sliced_info() equal to the host restatement before it looks at y; the data are integers and y must equal the exact result bit
for bit, over poisoned, over-long x, y and value arrays."""
import numpy as np
import pytest
import torch

import ladder as L
import ladder_sliced as LS
import spblas_reference_amd as sp
import test_gpu_sliced_ladders as T
from spblas_reference_amd import _capi

pytestmark = pytest.mark.gpu

PRE = T.PRE
VTS = ["f32", "f64"]
H, NB = 50, 64                      # rows per bin, bins
SHORT_RUNS = list(range(1, 6)) + [28] + list(range(29, 37)) + list(range(60, 69))
FAMILIES = ("items", "shares", "small_shares")
STORES = {"plain_stores": "0", "non_temporal_stores": "1"}


def _stretch(vt):
    return 2 * 64 // (LS.blk(vt) // 4)


def slice_blocks(vt):
    """Blocks per slice, 0 = an empty slice."""
    l_ = _stretch(vt)
    return [1, 0, 7, 8, 0, 0, 9, l_ - 1, l_, l_ + 1, 0, 16 * l_ - 1, 16 * l_, 16 * l_ + 1, 0, 2 * 16 * l_ + 1, 8 * l_ - 1, 8 * l_, 8 * l_ + 1]


def _runs_of_slice(vt, blocks, first, whole_last):
    """Run lengths (entries) of a slice of `blocks` blocks: the short runs from SHORT_RUNS[first] on while they fit, then runs of
    at most 32 blocks, the last one 3 entries short of its last block unless whole_last."""
    b, out, left, i = LS.blk(vt), [], blocks, first
    while left > 0 and len(out) < len(SHORT_RUNS):
        c = SHORT_RUNS[i % len(SHORT_RUNS)]
        if LS.cdiv(c, b) >= left:
            break
        out.append(c)
        left -= LS.cdiv(c, b)
        i += 1
    while left > 0:
        k = min(left, 32)        # (a bin's entries stay inside the LDS window of the value-free reduce)
        left -= k
        out.append(k * b - (0 if left or whole_last else 3))
    if not whole_last and blocks == 1:
        out = [b - 3]
    assert sum(LS.cdiv(c, b) for c in out) == blocks and len(out) <= NB
    return out


_FAM = {}


def family(kind, vt):
    key = (kind, vt)
    if key in _FAM:
        return _FAM[key]
    spec = slice_blocks(vt)
    if kind != "items":                  # even slices added: no slice above 3 x the mean any more
        spec = spec + [(26 if kind == "small_shares" else 30) * _stretch(vt) + k for k in range(14)]
    W = 64 if kind == "small_shares" else 4096
    last = max(s for s, nb in enumerate(spec) if nb)
    rows, cols, cnt = [], [], np.zeros((len(spec), NB), np.int64)
    for s, nb in enumerate(spec):
        for bin_, c in enumerate(_runs_of_slice(vt, nb, 3 * s, s == last)):
            r, cc = LS._tile(bin_, s, c, H, W, row0=s)
            rows.append(r)
            cols.append(cc)
            cnt[s, bin_] = c
    fam = LS.Family(f"expand_windows_{kind}", vt, NB * H, len(spec) * W, np.concatenate(rows), np.concatenate(cols),
                    LS._hooks(W, H), set(spec), spec=spec, cnt=cnt)
    # the family holds what it claims: the blocks per slice, every 16-byte phase at a slice's start and after a short run, and
    # a compact stream that ends with the last block
    t = fam.tiling()
    got = LS.tile_counts(fam.rowptr, fam.colind, t)
    assert t.S == len(spec) and t.NB == NB and np.array_equal(got, cnt)
    b = LS.blk(vt)
    assert list(LS.cdiv(got, b).sum(axis=1)) == spec
    item = LS.ITEM[vt]
    start = np.concatenate([[0], np.cumsum(((got + 3) & ~3).reshape(-1))])[:-1].reshape(got.shape)   # A' order: slice, bin
    populated = got > 0
    first_of_slice = {int(start[s][populated[s]][0] * item % 128) // 16 for s in range(t.S) if populated[s].any()}
    after_short = {int(start[s, j] * item % 128) // 16 for s in range(t.S) for j in range(1, NB)
                   if populated[s, j] and got[s, j - 1] in SHORT_RUNS}
    if item == 4:
        assert first_of_slice | after_short == set(range(8)) and len(after_short) == 8, (first_of_slice, after_short)
    else:  # fp64: runs are whole multiples of 4 entries = 32 bytes
        assert after_short == {0, 2, 4, 6}, after_short
    assert got[last][populated[last]][-1] % b == 0
    x_items = LS.work_lists(vt, got, t, fam.env)[0]
    assert (x_items > 0) == (kind == "items"), (kind, x_items)
    _FAM[key] = fam
    return fam


def _expand_grid(fam, cus):
    """(share, workgroups) of the equal-share expand: sliced_expand_typed restated."""
    t = fam.tiling()
    b = LS.blk(fam.vt)
    total = int(LS.cdiv(fam.meta["cnt"], b).sum())
    nwg = cus * (1 if t.W * LS.ITEM[fam.vt] > LS.constants()["PB_LDS_BYTES"] else 2)
    min_share = max(1, 2 * t.W // b)
    if nwg * min_share > total:
        nwg = max(total // min_share, min(t.S, nwg))
    share = LS.cdiv(total, max(nwg, 1))
    return share, LS.cdiv(total, share)


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("vt", VTS)
def test_expand_windows_snapshot(gpu, vt, kind, monkeypatch):
    """The snapshot plan (values inside the plan), plain and non-temporal product stores."""
    fam = family(kind, vt)
    dev = T.Dev(fam, np.int32, True)
    if kind != "items":
        share, wgs = _expand_grid(fam, T._cus())
        bounds = np.arange(1, wgs) * share
        edges = np.cumsum(fam.meta["spec"])
        assert np.setdiff1d(bounds, edges).size > 0, "no share boundary inside a slice"
        assert (share < _stretch(vt)) == (kind == "small_shares"), (kind, share)
        if kind == "shares":
            assert any(((edges > lo) & (edges < lo + share)).sum() >= 2 for lo in bounds), "no share spans a whole slice"
    for store, nt in STORES.items():
        info = T._inspect(dev, {PRE + "PB_NT": nt}, {"nt_product_stores": int(nt), "value_free": 0}, monkeypatch)
        assert (info.state_.info()["expand_items"] > 0) == (kind == "items")
        T._multiply(dev, info, {}, monkeypatch, f"{kind} {store}")


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("vt", VTS)
def test_expand_windows_value_free(gpu, vt, kind, monkeypatch):
    """The same tiles as value-free tiles (the expand gathers x alone), inspected with zeros and the values copied in
    afterwards; plain and non-temporal product stores."""
    fam = family(kind, vt)
    hooks = {k_: v_ for k_, v_ in fam.env.items() if k_ != PRE + "SLICE_ROWS"}
    for store, nt in STORES.items():
        dev = T.Dev(fam, np.int32, True, zero_values=True)
        full = dict(hooks, **{PRE + "PB_VFREE": "2", PRE + "PB_VF_ROWS": fam.env[PRE + "SLICE_ROWS"], PRE + "PB_NT": nt})
        for k_, v_ in full.items():
            monkeypatch.setenv(k_, v_)
        try:
            y = dev.new_y()
            info = sp.multiply_inspect(dev.a, dev.x, y, alg=_capi.SPMV_SLICED)
            pi, si = info.state_.info(), info.state_.sliced_info()
            assert pi["alg"] == _capi.SPMV_SLICED and si["value_free"] == 1 and si["nt_product_stores"] == int(nt), si
            pred = LS.predicted_info(vt, fam.rowptr, fam.colind, fam.shape, full, T._cus())
            got = dict(pi, **si)
            assert {k_: got[k_] for k_ in pred} == pred, {k_: (got[k_], pred[k_]) for k_ in pred if got[k_] != pred[k_]}
            dev.vals[:fam.nnz].copy_(L.cast(vt, dev.values))
            sp.multiply(info, dev.a, dev.x, y)
            dev.check(y, f"{kind} value-free {store}")
        finally:
            for k_ in full:
                monkeypatch.delenv(k_)


@pytest.mark.parametrize("vt", VTS)
def test_expand_windows_alpha_beta(gpu, vt, monkeypatch):
    """y = alpha A x + beta y through the C ABI, once: (-2, 0.5) over a y of small even integers."""
    fam = family("items", vt)
    dev = T.Dev(fam, np.int32, True)
    info = T._inspect(dev, {}, {}, monkeypatch)
    y0 = 2.0 * np.random.default_rng(8).integers(-3, 4, dev.m).astype(np.float64)
    y = dev.new_y()
    y.copy_(L.cast(vt, y0))
    T._capi_spmv(dev, info, -2.0, 0.5, y)
    ref = -2.0 * dev.ref + 0.5 * y0
    assert float((2.0 * dev.absrow + 0.5 * np.abs(y0)).max()) < 2 ** 23 and np.array_equal(ref * 2, np.round(ref * 2))
    dev.check(y, "alpha=-2 beta=0.5", ref=ref)


@pytest.mark.parametrize("vt", VTS)
def test_expand_windows_two_stages(gpu, vt, monkeypatch):
    """expand(), then reduce_rows in three ranges cut on bin boundaries, last range first."""
    fam = family("shares", vt)
    dev = T.Dev(fam, np.int32, True)
    info = T._inspect(dev, {}, {}, monkeypatch)
    m = dev.m
    cuts = [0, (NB // 3) * H, (2 * NB // 3) * H, m]
    y = dev.new_y()
    expand, reduce_rows = info.state_.bind_stages(dev.x, y.data_ptr(), dev.dt)
    expand()
    done = np.zeros(m, bool)
    for i in (2, 0, 1):
        reduce_rows(cuts[i], cuts[i + 1])
        done[cuts[i]:cuts[i + 1]] = True
        torch.cuda.synchronize()
        assert np.array_equal(~np.isnan(y.cpu().numpy()), done), f"range {i} wrote outside [{cuts[i]}, {cuts[i + 1]})"
    dev.check(y, "two stages, three ranges")
