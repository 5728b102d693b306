"""The ladders of tests/ladder.py checked without a GPU: the generators contain every rung they claim, the exact data sets stay
in the exact range, and the checkers bite -- a correct float64-derived output passes, the same output corrupted the way a
subtly wrong kernel would corrupt it fails.  Which check catches what (asserted below):

  corruption                                          random-data check      exact check
  last entry of a 65-entry row dropped                fails                  fails (the last entry whose product is not 0)
  one entry counted twice                             fails                  fails (an entry whose product is not 0)
  column n - 1 of C left at its old value             fails                  fails
  last n % 4 columns computed from the wrong B row    fails                  fails
  one sentinel of the padding overwritten             padding_untouched fails (bitwise, either data set)
  a 16-bit result rounded twice                       fails                  fails for bf16 (f16 holds the integers exactly)
"""
import numpy as np
import pytest
import torch

import ladder as L

VTS = ["f32", "f64", "c64", "c128", "f16", "bf16"]


_cast, _wide = L.cast, L.wide


def _spmv_case(vt, exact):
    rowptr, colind, shape = L.spmv_ladder()
    cplx = vt in ("c64", "c128")
    if exact:
        values, x = L.exact_spmv_data(rowptr, colind, shape[1], cplx=cplx, f16=vt == "f16")
    else:
        rng = np.random.default_rng(3)
        gen = L.random_complex if cplx else L.random_real
        values, x = gen(rng, colind.size), gen(rng, shape[1])
    values, x = _wide(_cast(vt, values)), _wide(_cast(vt, x))     # the inputs as the value type holds them
    ref, absrow = L.spmv_reference(rowptr, colind, values, x, shape)
    return rowptr, colind, shape, values, x, ref, absrow


# ------------------------------------------------------------------------------------------------- generators
def test_row_length_ladder_contains_every_rung():
    lens = set(L.row_lengths().tolist())
    assert set(range(0, 301)) <= lens
    for k in range(18):
        assert {(1 << k) - 1, 1 << k, (1 << k) + 1} <= lens, k
    th = L.thresholds()
    assert set(th) == {"window_f32", "window_f64", "window_c64", "window_c128", "window_lowp", "spmm_part_entries",
                       "spmm_cols_per_pass", "wave"}
    for name, t in th.items():
        assert t > 1 and {t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1} <= lens, name
    for lpr in L.lanes_per_row_steps():
        assert {lpr - 1, lpr, lpr + 1} <= lens
    assert max(lens) == (1 << 17) + 1
    rowptr, colind, shape = L.spmv_ladder()
    got = np.diff(rowptr)
    assert sorted(got.tolist()) == sorted(lens) and shape == (len(lens), L.SPMV_COLS)     # one row per length
    assert not np.array_equal(got, np.sort(got))                                         # ... in shuffled order
    assert colind.min() >= 0 and colind.max() < L.SPMV_COLS and colind.dtype == np.int32
    long_row = int(np.argmax(got))
    seg = colind[rowptr[long_row]:rowptr[long_row + 1]]
    assert np.unique(seg).size < seg.size and (np.diff(seg) < 0).any()                   # repeats, unsorted


def test_value_free_ladder_runs_up_to_the_lds_window():
    full = L.row_lengths()
    th = L.thresholds()
    for item in (4, 8):
        cap = L.value_free_window_cap(item)
        assert cap == (160 * 1024 - 64) // item - 8 * (1 + 64) - 16 and cap < 65535       # (the 65 536 limit is never the one)
        assert L.value_free_window_cap(item, 7) == cap - 8 * 6
        vf = L.value_free_row_lengths(item)
        assert set(full[full <= cap].tolist()) <= set(vf.tolist()) and {cap - 1, cap} <= set(vf.tolist()) and vf.max() == cap
        assert full[full > cap].min() > cap + 1 or cap + 1 in full           # cap + 1 is the fall-back case of the GPU test
        top = 15 if item == 4 else 14                                         # 2^15 + 1 in fp32, 2^14 + 1 in fp64 fit
        assert {(1 << top) - 1, 1 << top, (1 << top) + 1} <= set(vf.tolist()) and (1 << (top + 1)) > cap
        for w in ("window_f32", "window_f64", "spmm_part_entries"):
            assert {2 * th[w] - 1, 2 * th[w], 2 * th[w] + 1} <= set(vf.tolist())
        rowptr, _, shape = L.spmv_ladder(lengths=vf)
        assert sorted(np.diff(rowptr).tolist()) == vf.tolist() and shape[0] == vf.size
    short = L.short_row_lengths()
    assert short.max() == th["window_f32"] + 1 and set(range(0, 301)) <= set(short.tolist())
    assert np.array_equal(short, full[:short.size])


def test_capped_parts_matrix_reaches_the_cap():
    per, cap = L.spmm_parts_rule()
    rowptr, colind, (m, k) = L.spmm_capped_parts_matrix()
    lens = np.diff(rowptr)
    assert (per, cap) == (L.thresholds()["spmm_part_entries"], 64)
    assert -(-int(lens.max()) // per) > cap and (lens > per).sum() == 1 and colind.max() < k
    for f16 in (False, True):
        v, B = L.exact_spmm_data(rowptr, colind, (m, k), 257, f16=f16)
        r, a = L.spmm_reference(rowptr, colind, v, B, (m, k))
        assert a.max() < 2 ** 24 and np.array_equal(r, np.round(r))


def test_column_count_ladder_and_spmm_matrix_contain_what_they_claim():
    ns = L.SPMM_NS
    assert set(range(1, 161)) <= set(ns) and {191, 192, 255, 256, 257, 300, 511, 512, 513} <= set(ns) and len(set(ns)) == len(ns)
    th = L.thresholds()
    assert any(n > th["spmm_cols_per_pass"] and n % th["spmm_cols_per_pass"] for n in ns)   # n > 256, not a multiple of it
    for v in (2, 4):                                                                        # every width is reached and refused
        assert any(n % v == 0 for n in ns) and any(n % v for n in ns)
    rowptr, colind, (m, k) = L.spmm_matrix()
    lens = np.diff(rowptr)
    assert (m, k) == L.SPMM_SHAPE and 650 <= m <= 750 and 850 <= k <= 950
    assert (lens == 0).sum() >= 50 and set(range(1, 41)) <= set(lens.tolist())
    windows = [th[w] for w in ("window_f32", "window_f64", "window_c64", "window_c128", "window_lowp")]
    assert (lens > max(windows)).sum() == 3                                                # above every plan's window
    assert lens.max() > 2 * th["spmm_part_entries"] and lens.max() > 8192                   # parts > 1 (and > 2)
    b0, b1 = L.BAND_ROWS
    rows = np.repeat(np.arange(m), lens)[rowptr[b0]:rowptr[b1]]
    assert (b1 - b0) % 32 == 0 and b0 % 32 == 0 and (np.abs(colind[rowptr[b0]:rowptr[b1]] - rows) <= 20).all()
    assert set(L.LAYOUTS) == {"right", "right_ld+1", "right_ld+2", "right_ld+4", "left", "left_ld+1"}
    assert set(L.SHIFTS) == {(b, c) for b in (0, 1, 2) for c in (0, 1, 2)}


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("f16", [False, True])
def test_exact_data_sets_stay_in_the_exact_range(cplx, f16):
    rowptr, colind, shape = L.spmv_ladder()
    values, x = L.exact_spmv_data(rowptr, colind, shape[1], cplx=cplx, f16=f16)
    parts = lambda a: np.concatenate([a.real, a.imag]) if cplx else a
    assert set(np.unique(parts(values))) <= {-1.0, 0.0, 1.0} and set(np.unique(parts(x))) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    seq, anyorder = L.max_partial_sum(rowptr, colind, values, x)
    assert anyorder < 2 ** 24 and (not f16 or seq < 2 ** 11)
    ref, _ = L.spmv_reference(rowptr, colind, values, x, shape)
    assert np.array_equal(parts(ref), np.round(parts(ref))) and np.abs(parts(ref)).max() > 100   # integers, not all tiny
    if f16:
        assert np.abs(parts(ref)).max() < 2 ** 11
        assert np.array_equal(torch.as_tensor(parts(ref)).to(torch.float16).double().numpy(), parts(ref))
    rp2, ci2, sh2 = L.spmm_matrix()
    v2, B = L.exact_spmm_data(rp2, ci2, sh2, 64, cplx=cplx, f16=f16)
    assert set(np.unique(parts(v2))) <= {-1.0, 0.0, 1.0} and np.abs(parts(B)).max() <= 2
    r2, a2 = L.spmm_reference(rp2, ci2, v2, B, sh2)
    assert np.array_equal(parts(r2), np.round(parts(r2))) and a2.max() < 2 ** 24
    if f16:
        assert np.abs(parts(r2)).max() < 2 ** 11


def test_max_partial_sum_sees_a_peak_inside_a_row():
    rowptr = np.array([0, 0, 4, 6], dtype=np.int64)
    colind = np.array([0, 1, 2, 3, 0, 1], dtype=np.int32)
    values = np.array([1.0, 1.0, -1.0, -1.0, 1.0, -1.0])
    x = np.array([2.0, 2.0, 2.0, 2.0])
    assert L.max_partial_sum(rowptr, colind, values, x) == (4.0, 8.0)    # the row sums to 0, its prefix reaches 4


# ------------------------------------------------------------------------------------------------- checkers: SpMV
@pytest.mark.parametrize("vt", VTS)
def test_spmv_checkers_pass_the_correct_output_and_fail_a_dropped_or_doubled_entry(vt):
    for exact in (False, True):
        rowptr, colind, shape, values, x, ref, absrow = _spmv_case(vt, exact)
        lens = np.diff(rowptr)
        good = _cast(vt, ref)
        run = (lambda y, w: L.check_exact(vt, y, ref, w)) if exact else \
            (lambda y, w: L.check_random(vt, y, ref, absrow, lens, w))
        run(good, "correct output")
        r65 = int(np.flatnonzero(lens == 65)[0])
        prods = values[rowptr[r65]:rowptr[r65 + 1]] * x[colind[rowptr[r65]:rowptr[r65 + 1]]]
        nz = np.flatnonzero(prods != 0)
        # the LAST entry of the row whose product is not 0 (the very last one where it is not 0: always so for the random set;
        # about half the products of the integer set are 0, and dropping one of those changes nothing), and an earlier one
        assert nz.size > 8 and (exact or nz[-1] == 64)
        for name, delta in (("last (non-zero) entry of the 65-entry row dropped", -prods[nz[-1]]),
                            ("one entry counted twice", prods[nz[3]])):
            bad = ref.copy()
            bad[r65] += delta
            with pytest.raises(AssertionError):
                run(_cast(vt, bad), name)
        nan = good.clone()
        nan[3] = float("nan")          # a row the kernel never wrote (y is prefilled with NaN)
        with pytest.raises(AssertionError):
            run(nan, "row never written")


# ------------------------------------------------------------------------------------------------- checkers: SpMM
def _spmm_case(vt, exact, n):
    rowptr, colind, shape = L.spmm_matrix()
    cplx = vt in ("c64", "c128")
    if exact:
        values, B = L.exact_spmm_data(rowptr, colind, shape, n, cplx=cplx, f16=vt == "f16")
    else:
        rng = np.random.default_rng(4)
        gen = L.random_complex if cplx else L.random_real
        values, B = gen(rng, colind.size), gen(rng, (shape[1], n))
    values, B = _wide(_cast(vt, values)), _wide(_cast(vt, B))
    ref, absr = L.spmm_reference(rowptr, colind, values, B, shape)
    return rowptr, colind, shape, values, B, ref, absr


@pytest.mark.parametrize("vt", VTS)
def test_spmm_checkers_fail_a_stale_last_column_and_a_tail_from_the_wrong_b_row(vt):
    n = 37                                                      # n % 4 == 1: the scalar tail after the 4-wide lanes
    for exact in (False, True):
        rowptr, colind, shape, values, B, ref, absr = _spmm_case(vt, exact, n)
        lens = np.diff(rowptr)
        run = (lambda C, w: L.check_exact(vt, C, ref, w)) if exact else \
            (lambda C, w: L.check_random(vt, C, ref, absr, lens, w))
        run(_cast(vt, ref), "correct output")
        stale = _cast(vt, ref).clone()
        stale[:, n - 1] = L.SENTINEL[L.TORCH_OF[vt]]            # column n - 1 left at its old value
        with pytest.raises(AssertionError):
            run(stale, "column n - 1 left at its old value")
        wrong, _ = L.spmm_reference(rowptr, colind, values, np.roll(B, 1, axis=0), shape)   # B row k - 1 instead of k
        tail = ref.copy()
        tail[:, n - n % 4:] = wrong[:, n - n % 4:]
        assert n % 4 == 1 and not np.array_equal(tail, ref)
        with pytest.raises(AssertionError):
            run(_cast(vt, tail), "last n % 4 columns from the wrong B row")


@pytest.mark.parametrize("dt", [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.complex64, torch.complex128])
@pytest.mark.parametrize("layout", L.LAYOUTS)
def test_a_single_overwritten_sentinel_is_seen(dt, layout):
    rows, cols = 7, 5
    for shift in (0, 1, 2):
        store, view, mask = L.dense_window(rows, cols, layout, shift, dt, "cpu")
        assert view.shape == (rows, cols) and int(mask.sum()) == rows * cols and view.storage_offset() == shift
        pad = int(layout.split("+")[1]) if "+" in layout else 0
        assert (view.stride(0) == 1 and view.stride(1) == rows + pad) if layout.startswith("left") else \
            (view.stride(1) == 1 and view.stride(0) == cols + pad)
        view.copy_(torch.arange(rows * cols, dtype=torch.float64).reshape(rows, cols).to(dt))   # the library writes the view
        assert L.padding_untouched(store, mask, dt)
        outside = (~mask).nonzero().flatten()
        assert outside.numel() >= 8 + shift
        for pos in (outside[0], outside[outside.numel() // 2], outside[-1]):
            s2 = store.clone()
            s2[pos] = 0.0                                                                      # one element of the padding
            assert not L.padding_untouched(s2, mask, dt), (layout, shift, int(pos))
        if dt in (torch.float32, torch.float64):
            s2 = store.clone()
            s2[outside[0]] = torch.nextafter(s2[outside[0]], torch.tensor(0.0, dtype=dt))               # one ulp off
            assert not L.padding_untouched(s2, mask, dt)


@pytest.mark.parametrize("vt", ["f16", "bf16"])
def test_a_16_bit_result_rounded_twice_fails(vt):
    """y = alpha * A x + beta * y0 with the product rounded to 16 bits BEFORE the beta term is added (two roundings where the
    kernels keep fp32 until the end)."""
    dt = L.TORCH_OF[vt]
    for exact in (False, True):
        rowptr, colind, shape, values, x, ref, absrow = _spmv_case(vt, exact)
        lens = np.diff(rowptr)
        rng = np.random.default_rng(8)
        y0 = _wide(_cast(vt, rng.integers(-300, 300, ref.shape).astype(np.float64) if exact else rng.uniform(-1, 1, ref.shape)))
        total, tabs = ref + y0, absrow + np.abs(y0)
        once = _cast(vt, total)
        twice = (torch.as_tensor(ref).to(dt).double() + torch.as_tensor(y0)).to(dt)
        if exact:
            L.check_exact(vt, once, total, "rounded once")
            if vt == "bf16":     # integers above 256 do not fit 8 bits: the early rounding shows
                with pytest.raises(AssertionError):
                    L.check_exact(vt, twice, total, "rounded twice")
            else:                # f16 holds every integer of this data set: both roundings are exact, nothing differs
                assert L.bits_equal(twice, total, dt)
        else:
            L.check_random(vt, once, total, tabs, lens, "rounded once")
            with pytest.raises(AssertionError):
                L.check_random(vt, twice, total, tabs, lens, "rounded twice")
