"""-m gpu: the tile ladders of the SLICED SpMV plan (tests/ladder_sliced.py has the families, the restated tiling and the host
model; tests/test_ladders_sliced_cpu.py proves on the host that the families hold their rungs and the checkers bite).

Every case first asserts that the plan is SLICED and that plan.info() / plan.sliced_info() equal the restated tiling
(predicted_info) -- a case cannot pass while missing its rung -- and then runs twice: integer data whose result must equal
the float64 sum rounded once, bit for bit (ladder.check_exact), and random data under the existing bound of the value type
(ladder.check_random).  y is prefilled with NaN; every array is longer than it has to be, with NaN behind the values, x and y
and a wild column behind colind, and what lies behind y must still be NaN afterwards.  No case skips.
"""
import ctypes

import numpy as np
import pytest
import torch

import ladder as L
import ladder_sliced as LS
import spblas_reference_amd as sp
from spblas_reference_amd import _capi

pytestmark = pytest.mark.gpu

VTS = ["f32", "f64"]
OFFSETS = {"o32": np.int32, "o64": np.int64}
SLACK, WILD = 64, 2 ** 30
PRE = "SPBLAS_GFX950_"
# plan name -> (hooks of the inspect call, what sliced_info() must report)
VARIANTS = {"default": ({}, {}),
            "one_byte_codes": ({PRE + "PB_ENC8": "2"}, {"row_code_u8": 1}),
            "ksplit_4": ({PRE + "PB_KSPLIT": "4"}, {"ksplit": 4}),
            "direct_scatter": ({PRE + "PB_STAGED_SCATTER": "0"}, {"row_code_u8": 0}),
            "plain_stores": ({PRE + "PB_NT": "0"}, {"nt_product_stores": 0}),
            "non_temporal_stores": ({PRE + "PB_NT": "1"}, {"nt_product_stores": 1})}

_FAMILIES = {}


def _family(name, vt):
    """Families by name, built once per session (host arrays; never written to)."""
    key = (name, vt)
    if key not in _FAMILIES:
        if name.startswith("col_edges_"):
            f = LS.col_edges(vt, name[len("col_edges_"):])
        elif name.startswith("row_edges_"):
            f = LS.row_edges(vt, name[len("row_edges_"):])
        elif name == "row_codes_overflow":
            f = LS.row_codes(vt, overflow=True)
        elif name.startswith("bin_span_"):
            f = LS.bin_span_family(vt, int(name[len("bin_span_"):]))
        elif name in ("slice_aligned", "many_groups"):       # built for the CU count of the device
            f = getattr(LS, name)(vt, _cus())
        else:
            f = getattr(LS, name)(vt)
        assert f.name == name
        _FAMILIES[key] = f
    return _FAMILIES[key]


FAMILY_NAMES = ["runs", "dups", "row_codes", "row_codes_overflow", "many_slices", "hub_rows", "hub_len", "split_rows",
                "compact_rows", "skew_cols", "skew_rows", "many_groups"] + [f"bin_span_{s_}" for s_ in LS.BIN_SPANS] + \
    ["col_edges_" + c for c in LS.COL_EDGE_CASES] + ["row_edges_" + c for c in LS.ROW_EDGE_CASES]
LADDER_CASES = [(vt_, n_) for vt_ in VTS for n_ in FAMILY_NAMES] + [("f64", "slice_aligned")]
# variants some families run on top of VARIANTS: the work lists in list order, positions staged as 32-bit words
LPT_OFF = {"lists_in_list_order": ({PRE + "PB_LPT": "0"}, {})}
EXTRA_VARIANTS = dict({n_: LPT_OFF for n_ in ("skew_cols", "skew_rows", "many_groups")},
                      **{f"bin_span_{s_}": {"wide_staging": ({PRE + "PB_STAGE_Q16": "0"}, {})} for s_ in LS.BIN_SPANS})
# which list a family must report (predicted_info says how long; here: that it is there at all)
WORK_LIST = {"skew_cols": "expand_items", "skew_rows": "reduce_items", "many_groups": "reduce_items",
             "slice_aligned": "expand_items"}

_HOST = {}


def _host_data(fam, exact):
    """(values, x, reference, sum |a||x| per row) as float64, the inputs rounded to the value type; computed once per family
    and data set and shared by every case.  Integer data: every partial sum in any order stays exact (asserted)."""
    key = (fam.name, fam.vt, exact)
    if key not in _HOST:
        n = fam.shape[1]
        if exact:
            values, x = LS.exact_data(fam)
        else:
            rng = np.random.default_rng(12)
            values, x = L.random_real(rng, fam.nnz), L.random_real(rng, n)
        values, x = L.wide(L.cast(fam.vt, values)), L.wide(L.cast(fam.vt, x))
        if exact:
            seq, anyorder = L.max_partial_sum(fam.rowptr, fam.colind, values, x)
            assert anyorder < 2 ** 24 and seq < 2 ** 24
        _HOST[key] = (values, x) + tuple(L.spmv_reference(fam.rowptr, fam.colind, values, x, fam.shape))
    return _HOST[key]


class Dev:
    """A family on the device: over-long, poisoned arrays and the csr_view over them."""

    def __init__(self, fam, offsets, exact, zero_values=False):
        self.fam, self.exact = fam, exact
        self.m, self.n = fam.shape
        self.values, self.x_host, self.ref, self.absrow = _host_data(fam, exact)
        dt = L.TORCH_OF[fam.vt]
        self.dt = dt
        vals = torch.full((fam.nnz + SLACK,), float("nan"), dtype=dt)
        vals[:fam.nnz] = L.cast(fam.vt, np.zeros(fam.nnz) if zero_values else self.values)
        ci = torch.full((fam.nnz + SLACK,), WILD, dtype=torch.int32)
        ci[:fam.nnz] = torch.from_numpy(fam.colind)
        rp = torch.full((self.m + 1 + SLACK,), -7, dtype=torch.from_numpy(np.zeros(1, offsets)).dtype)
        rp[:self.m + 1] = torch.from_numpy(fam.rowptr.astype(offsets))
        xb = torch.full((self.n + SLACK,), float("nan"), dtype=dt)
        xb[:self.n] = L.cast(fam.vt, self.x_host)
        self.vals, self.ci, self.rp, self.xb = vals.cuda(), ci.cuda(), rp.cuda(), xb.cuda()
        self.x = self.xb[:self.n]
        self.a = sp.csr_view(self.vals, self.rp, self.ci, fam.shape, fam.nnz)
        self.lens = np.diff(fam.rowptr)

    def new_y(self, fill=float("nan")):
        self.yb = torch.full((self.m + SLACK,), float("nan"), dtype=self.dt, device="cuda")
        self.yb[:self.m] = fill
        return self.yb[:self.m]

    def set_values(self, values):
        """New values written in place (float64 numbers the value type holds); the reference follows."""
        self.values = L.wide(L.cast(self.fam.vt, values))
        self.vals[:self.fam.nnz].copy_(L.cast(self.fam.vt, self.values))
        self.ref, self.absrow = L.spmv_reference(self.fam.rowptr, self.fam.colind, self.values, self.x_host, self.fam.shape)

    def check(self, y, what, ref=None, absrow=None):
        torch.cuda.synchronize()
        what = f"{self.fam.name} {self.fam.vt} {what} {'exact' if self.exact else 'random'}"
        assert bool(torch.isnan(self.yb[self.m:]).all()), f"{what}: the multiply wrote behind y"
        ref = self.ref if ref is None else ref
        if self.exact:
            L.check_exact(self.fam.vt, y, ref, what)
        else:
            L.check_random(self.fam.vt, y, ref, self.absrow if absrow is None else absrow, self.lens, what)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _inspect(dev, env, want, monkeypatch, **kw):
    """multiply_inspect under the family's geometry hooks + `env`; the plan must be SLICED and report the restated tiling."""
    fam = dev.fam
    full = dict(fam.env, **env)
    for k_, v_ in full.items():
        monkeypatch.setenv(k_, v_)
    try:
        info = sp.multiply_inspect(dev.a, dev.x, dev.new_y(), alg=_capi.SPMV_SLICED, **kw)
    finally:
        for k_ in full:
            monkeypatch.delenv(k_)
    pi, si = info.state_.info(), info.state_.sliced_info()
    assert pi["alg"] == _capi.SPMV_SLICED, f"{fam.name}: forced SLICED ended up as {pi['alg']}"
    pred = LS.predicted_info(fam.vt, fam.rowptr, fam.colind, fam.shape, full, _cus())
    got = dict(pi, **si)
    assert {k_: got[k_] for k_ in pred} == pred, (fam.name, env, {k_: (got[k_], pred[k_]) for k_ in pred if got[k_] != pred[k_]})
    assert all(si[k_] == v_ for k_, v_ in want.items()), (fam.name, env, want, si)
    return info


def _multiply(dev, info, env, monkeypatch, what):
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    try:
        y = dev.new_y()
        sp.multiply(info, dev.a, dev.x, y)
        dev.check(y, what)
    finally:
        for k_ in env:
            monkeypatch.delenv(k_)


# ===================================================================================================== groups per bin
@pytest.mark.parametrize("scatter", ["staged", "direct"])
@pytest.mark.parametrize("rwaves", ["4", "8"])
@pytest.mark.parametrize("rows", ["two_byte_rows", "one_byte_codes"])
@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_groups_per_bin_ladder(gpu, vt, offsets, rows, rwaves, scatter, monkeypatch):
    """One bin per group count 0 ... 34 through every batch depth and every K split of the reduce, on one plan per row
    encoding x wave-bins per workgroup x scatter.  PB_RBATCH and PB_KSPLIT are read per call: 16 multiplies per plan and data
    set, no re-inspect.  The direct scatter never leaves the runs sorted, so it must report 16-bit rows even when one-byte
    codes are asked for."""
    fam = _family("groups", vt)
    env = {PRE + "PB_ENC8": "2" if rows == "one_byte_codes" else "0", PRE + "PB_RWAVES": rwaves,
           PRE + "PB_STAGED_SCATTER": "1" if scatter == "staged" else "0"}
    want = {"row_code_u8": int(rows == "one_byte_codes" and scatter == "staged")}
    ran = 0
    for exact in (True, False):
        dev = Dev(fam, OFFSETS[offsets], exact)
        info = _inspect(dev, env, want, monkeypatch)
        for ub in ("1", "2", "4", "8"):
            for k in ("1", "2", "3", "4"):
                _multiply(dev, info, {PRE + "PB_RBATCH": ub, PRE + "PB_KSPLIT": k}, monkeypatch,
                          f"{rows} RW={rwaves} {scatter} UB={ub} K={k}")
                ran += 1
    assert ran == 32


# ================================================================================================ every other family
@pytest.mark.parametrize("vt,name", LADDER_CASES)
@pytest.mark.parametrize("offsets", list(OFFSETS))
def test_tile_ladder(gpu, vt, offsets, name, monkeypatch):
    """Every family through the default plan, forced one-byte codes, K = 4, the direct scatter and both product-store
    flavours.  row_codes_overflow holds a bin with PB_EXC_CAP + 1 exceptions: asked for one-byte codes it must come back with
    16-bit rows; many_slices has more slices than the staged scatter takes and must scatter directly (16-bit rows) unasked;
    the runs of bin_span are longer than the staging area of the ordered scatter, so the encoding it ends up with is not
    asserted there.
    skew_cols / skew_rows: a slice / a group of bins above 3 x the mean -- the heavy slice cut into parts for the expand (also
    with non-temporal stores), the heavy group's streams cut in two for the reduce, whose partial rows
    pb_combine_items_kernel adds; PB_LPT=0 leaves the expand's list in slice order (the reduce's list of 6 items is never
    sorted).  many_groups: variable bins in more groups than 2 x the CUs -- the reduce's list IS sorted heaviest first, with
    split groups, the scatter takes the bins heaviest first, and PB_LPT=0 leaves both in order.  bin_span: a bin whose rows
    span 65 535, 65 536 and 65 537 entries of the caller's arrays; the staged scatter keeps positions as 16-bit words below
    65 536 (PB_STAGE_Q16=0: never).  slice_aligned: fp64 at the natural width, the slice count rounded up to the CU count and
    one expand item per slice."""
    fam = _family(name, vt)
    variants = dict(VARIANTS, **EXTRA_VARIANTS.get(name, {}))
    ran = set()
    for exact in (True, False):
        dev = Dev(fam, OFFSETS[offsets], exact)
        for variant, (env, want) in variants.items():
            want = dict(want)
            if "row_code_u8" in want and name in ("row_codes_overflow", "many_slices"):
                want["row_code_u8"] = 0
            if name.startswith("bin_span_"):
                want.pop("row_code_u8", None)
            info = _inspect(dev, env, want, monkeypatch)
            pi = info.state_.info()
            if name == "many_slices":
                assert pi["n_slices"] > LS.constants()["PB_STAGE_MAX_S"]
            if name in WORK_LIST:
                assert pi[WORK_LIST[name]] > 0, (name, variant, pi)
            if name == "slice_aligned":
                assert pi["n_slices"] == _cus() == pi["expand_items"]
            if name == "many_groups":
                si = info.state_.sliced_info()
                assert si["variable_bins"] == 1 and si["n_bins"] > 2 * _cus() and pi["reduce_items"] > LS.cdiv(si["n_bins"], 4) > 2 * _cus()
            _multiply(dev, info, env, monkeypatch, variant)
            ran.add(variant)
    assert ran == set(variants)


# =============================================================================================================== hot split
@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_tile_ladder_hot_split(gpu, vt, offsets, monkeypatch):
    """PB_HOT=1 on the family whose hot columns the sample must take: hot_split reports exactly those columns and their
    entries, hot_entries + tiled_entries == nnz, and the tile numbers are those of A_rest restated on the host.  Through
    the default plan, one-byte codes, K = 4, the direct scatter and both product-store flavours; then new values (the plan
    builds both halves again); then two stages: all rows in one reduce, a proper row range refused."""
    fam = _family("hot_split", vt)
    hot_per_row = fam.meta["hot_per_row"]
    rest_rowptr, rest_colind = fam.meta["rest"]
    for exact in (True, False):
        dev = Dev(fam, OFFSETS[offsets], exact)
        for variant, (env, want) in VARIANTS.items():
            full = dict(fam.env, **env)
            for k_, v_ in full.items():
                monkeypatch.setenv(k_, v_)
            try:
                info = sp.multiply_inspect(dev.a, dev.x, dev.new_y(), alg=_capi.SPMV_SLICED)
                pi, si = info.state_.info(), info.state_.sliced_info()
                assert pi["alg"] == _capi.SPMV_SLICED and "hot_split" in si, si
                assert all(si[k_] == v_ for k_, v_ in want.items()), (variant, want, si)
                hs = si["hot_split"]
                assert hs["hot_columns"] == len(LS.HOT_COLS) and hs["hot_entries"] == int(hot_per_row.sum())
                assert hs["hot_entries"] + hs["tiled_entries"] == fam.nnz and hs["hot_rows"] == int((hot_per_row > 0).sum())
                pred = LS.predicted_info(vt, rest_rowptr, rest_colind, fam.shape, full, _cus())
                got = dict(pi, **si)
                assert {k_: got[k_] for k_ in pred} == pred, {k_: (got[k_], pred[k_]) for k_ in pred if got[k_] != pred[k_]}
                y = dev.new_y()
                sp.multiply(info, dev.a, dev.x, y)
                dev.check(y, f"hot split, {variant}")
                if variant == "default":
                    dev.set_values(dev.values[::-1] * (2.0 if exact else 0.5))
                    info.state_.update_values(dev.a.values())
                    assert "hot_split" in info.state_.sliced_info()
                    y = dev.new_y()
                    sp.multiply(info, dev.a, dev.x, y)
                    dev.check(y, "hot split, new values")
                    y = dev.new_y()
                    expand, reduce_rows = info.state_.bind_stages(dev.x, y.data_ptr(), dev.dt)
                    expand()
                    reduce_rows(0, dev.m)
                    dev.check(y, "hot split, two stages")
                    with pytest.raises(sp.BackendError):
                        reduce_rows(0, dev.m // 2)
            finally:
                for k_ in full:
                    monkeypatch.delenv(k_)


# ======================================================================================================= value-free tiles
@pytest.mark.parametrize("waves", ["4", "8"])
@pytest.mark.parametrize("name", ["runs", "groups", "dups"] + ["col_edges_" + c for c in LS.COL_EDGE_CASES])
@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_tile_ladder_value_free(gpu, vt, offsets, name, waves, monkeypatch):
    """The same tiles read through the value-free reduce (a plain inspected csr_view; PB_VFREE=2 builds it for small
    matrices): the bin height comes through PB_VF_ROWS because SLICE_ROWS switches value-free tiles off.  Inspected with zeros,
    the data copied in afterwards: the plan must read the caller's values at the time of the call."""
    fam = _family(name, vt)
    hooks = {k_: v_ for k_, v_ in fam.env.items() if k_ != PRE + "SLICE_ROWS"}
    env = dict(hooks, **{PRE + "PB_VFREE": "2", PRE + "PB_VF_ROWS": fam.env[PRE + "SLICE_ROWS"], PRE + "PB_VF_WAVES": waves})
    for rows, enc in (("two_byte_rows", "0"), ("one_byte_codes", "2")):
        for exact in (True, False):
            dev = Dev(fam, OFFSETS[offsets], exact, zero_values=True)
            full = dict(env, **{PRE + "PB_ENC8": enc})
            for k_, v_ in full.items():
                monkeypatch.setenv(k_, v_)
            try:
                y = dev.new_y()
                info = sp.multiply_inspect(dev.a, dev.x, y, alg=_capi.SPMV_SLICED)
                pi, si = info.state_.info(), info.state_.sliced_info()
                assert pi["alg"] == _capi.SPMV_SLICED and si["value_free"] == 1 and si["row_code_u8"] == int(enc == "2"), si
                pred = LS.predicted_info(vt, fam.rowptr, fam.colind, fam.shape, full, _cus())
                got = dict(pi, **si)
                assert {k_: got[k_] for k_ in pred} == pred, {k_: (got[k_], pred[k_]) for k_ in pred if got[k_] != pred[k_]}
                dev.vals[:fam.nnz].copy_(L.cast(vt, dev.values))
                sp.multiply(info, dev.a, dev.x, y)
                dev.check(y, f"value-free, {waves} waves, {rows}")
            finally:
                for k_ in full:
                    monkeypatch.delenv(k_)


# ================================================================================================================ values
@pytest.mark.parametrize("mode", ["rebuild_on_first_update", "update_bins", "update_gather", "keep_src_hook"])
@pytest.mark.parametrize("name", ["runs", "dups", "col_edges_asked_100_gets_96"])
@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_tile_ladder_new_values(gpu, vt, offsets, name, mode, monkeypatch):
    """After the first multiply the values are rewritten in place and the plan refreshed with update_values, twice: a snapshot
    plan holds no source positions and builds itself again on its first update (`rebuild_on_first_update`); a plan told that
    the values will change gathers bin by bin through LDS (`update_bins`) or in A' order (PB_UPDATE_BINS=0, `update_gather`);
    PB_KEEP_SRC=1 keeps the positions from the start without being told.  What tells them apart is device_bytes: the source
    positions and the run table (ladder_sliced.source_position_bytes) are there from the start in the last three modes and
    appear with the first update -- the second build -- in the first."""
    fam = _family(name, vt)
    t = fam.tiling()
    src_bytes = LS.source_position_bytes(vt, LS.tile_counts(fam.rowptr, fam.colind, t), t)
    assert src_bytes >= 4 * fam.nnz
    for exact in (True, False):
        dev = Dev(fam, OFFSETS[offsets], exact)
        env = {PRE + "PB_KEEP_SRC": "1"} if mode == "keep_src_hook" else {}
        call_env = {PRE + "PB_UPDATE_BINS": "0"} if mode == "update_gather" else {}
        plain_bytes = _inspect(dev, {}, {}, monkeypatch).state_.info()["device_bytes"]       # a snapshot plan without positions
        info = _inspect(dev, env, {}, monkeypatch, values_will_change=mode in ("update_bins", "update_gather"))
        kept_from_start = mode != "rebuild_on_first_update"
        assert info.state_.info()["device_bytes"] == plain_bytes + (src_bytes if kept_from_start else 0), mode
        _multiply(dev, info, {}, monkeypatch, f"{mode}: first values")
        base = dev.values
        for round_, factor in enumerate((-2.0, 3.0)):
            perm = np.random.default_rng(40 + round_).permutation(fam.nnz)
            dev.set_values(base[perm] * factor if exact else base[perm] * 0.5 * factor)
            full = dict(fam.env, **env, **call_env)      # (a plan that builds itself again must meet the same hooks)
            for k_, v_ in full.items():
                monkeypatch.setenv(k_, v_)
            try:
                info.state_.update_values(dev.a.values())
            finally:
                for k_ in full:
                    monkeypatch.delenv(k_)
            pred = LS.predicted_info(vt, fam.rowptr, fam.colind, fam.shape, fam.env, _cus())
            got = dict(info.state_.info(), **info.state_.sliced_info())
            assert {k_: got[k_] for k_ in pred} == pred, (mode, got)
            assert info.state_.info()["alg"] == _capi.SPMV_SLICED
            assert info.state_.info()["device_bytes"] == plain_bytes + src_bytes, (mode, round_)
            _multiply(dev, info, {}, monkeypatch, f"{mode}: values of round {round_ + 1}")


# ============================================================================================================ alpha / beta
def _capi_spmv(dev, info, alpha, beta, y):
    ct = ctypes.c_float if dev.fam.vt == "f32" else ctypes.c_double
    a_, b_ = ct(alpha), ct(beta)
    hd = sp.api._Handle.current(y.device)
    sp.api.check(_capi.lib().spblas_gfx950_spmv(hd.h, info.state_.plan, _capi.OP_N, dev.m, dev.n, dev.fam.nnz, ctypes.byref(a_),
                                                sp.api._ptr(dev.rp), sp.api._ptr(dev.ci), sp.api._ptr(dev.vals),
                                                sp.api._ptr(dev.x), ctypes.byref(b_), sp.api._ptr(y),
                                                sp.api._OT[dev.rp.dtype], sp.api._VT[dev.dt][0]), "spmv")


@pytest.mark.parametrize("name", ["runs", "dups", "row_edges_empty_bins", "row_edges_m_kH_plus_1"])
@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_tile_ladder_alpha_beta(gpu, vt, offsets, name, monkeypatch):
    """y = alpha A x + beta y through the C ABI with (1, 0), (-2, 0.5) and (0.5, 1) over a y of small even integers (every
    term stays an integer or a half: still exact); with beta = 0, y starts as NaN and must not be read."""
    fam = _family(name, vt)
    for exact in (True, False):
        dev = Dev(fam, OFFSETS[offsets], exact)
        info = _inspect(dev, {}, {}, monkeypatch)
        y0 = 2.0 * np.random.default_rng(8).integers(-3, 4, dev.m).astype(np.float64)
        for alpha, beta in ((1.0, 0.0), (-2.0, 0.5), (0.5, 1.0)):
            y = dev.new_y()
            if beta != 0.0:
                y.copy_(L.cast(vt, y0))
            _capi_spmv(dev, info, alpha, beta, y)
            ref = alpha * dev.ref + (beta * y0 if beta != 0.0 else 0.0)
            absrow = abs(alpha) * dev.absrow + abs(beta) * np.abs(y0) * (beta != 0.0)
            if exact:
                assert float(np.abs(absrow).max()) < 2 ** 23 and np.array_equal(ref * 2, np.round(ref * 2))
            dev.check(y, f"alpha={alpha} beta={beta}", ref=ref, absrow=absrow)


# ============================================================================================================== two stages
@pytest.mark.parametrize("name", ["runs", "row_edges_empty_bins", "row_edges_m_kH_plus_1", "col_edges_empty_slices"])
@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_tile_ladder_two_stages(gpu, vt, offsets, name, monkeypatch):
    """expand(), then reduce_rows over [0, m) in one call and in three ranges cut on bin boundaries, last range first: the
    rows of the ranges not reduced yet stay NaN until their call."""
    fam = _family(name, vt)
    for exact in (True, False):
        dev = Dev(fam, OFFSETS[offsets], exact)
        info = _inspect(dev, {}, {}, monkeypatch)
        H, NB, m = info.state_.info()["rows_per_bin"], info.state_.sliced_info()["n_bins"], dev.m
        assert NB >= 3
        y = dev.new_y()
        expand, reduce_rows = info.state_.bind_stages(dev.x, y.data_ptr(), dev.dt)
        expand()
        reduce_rows(0, m)
        dev.check(y, "two stages, one range")
        cuts = [0, (NB // 3) * H, (2 * NB // 3) * H, m]
        y = dev.new_y()
        expand, reduce_rows = info.state_.bind_stages(dev.x, y.data_ptr(), dev.dt)
        expand()
        done = np.zeros(m, bool)
        for i in (2, 0, 1):
            reduce_rows(cuts[i], cuts[i + 1])
            done[cuts[i]:cuts[i + 1]] = True
            torch.cuda.synchronize()
            assert np.array_equal(~np.isnan(y.cpu().numpy()), done), f"{name}: range {i} wrote outside [{cuts[i]}, {cuts[i + 1]})"
        dev.check(y, "two stages, three ranges")


@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("vt", VTS)
def test_tile_ladder_two_stages_refuse_a_row_range_of_split_rows(gpu, vt, offsets, monkeypatch):
    """The pieces of a split row lie in different bins and their sums only meet when every bin has been reduced: all rows in
    one reduce_rows call work, a proper row range is refused (documented)."""
    fam = _family("split_rows", vt)
    dev = Dev(fam, OFFSETS[offsets], True)
    info = _inspect(dev, {}, {}, monkeypatch)
    y = dev.new_y()
    expand, reduce_rows = info.state_.bind_stages(dev.x, y.data_ptr(), dev.dt)
    expand()
    reduce_rows(0, dev.m)
    dev.check(y, "split rows, two stages")
    with pytest.raises(sp.BackendError) as e:
        reduce_rows(0, dev.m // 2)
    assert e.value.status == _capi.NOT_SUPPORTED
