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


# ===================================================================================================== SpGEMM / add ladder
"""Host proofs of the SpGEMM / add ladder: every rung is in every family and sits in the bin / on the path it is meant for; the
columns of the adversarial rungs hash where they claim; the exact data stay exact; the numpy reference equals the CPU oracle;
the checkers fail a dropped product, a doubled one, two swapped columns, a value on the neighbouring entry, a row offset off by
one."""
SPG_FAMILIES = L.spg_families()
SPG_IDS = [f"sub{s}_a{a}" for s, a in SPG_FAMILIES]


def test_spgemm_thresholds_and_their_restatement():
    t = L.spg_thresholds()
    assert t["bin_limits"] == sorted(t["bin_limits"]) and len(t["bin_limits"]) == 4
    for b, T in enumerate(t["bin_limits"], start=1):
        assert L.bin_of([T - 1, T, T + 1]).tolist() == [b if T > 1 else 0, b, b + 1]
        assert (1 << t["log2hs"][b]) == 2 * T                         # every table is twice its bin's limit
    assert L.bin_of([0, 1]).tolist() == [0, 1]
    assert t["rank_caps"] == t["bin_limits"][1:3]                     # a byte / two bytes hold the ranks of bins 1-2 / 3
    assert t["cap"] == t["sort_products"] and t["cap_add"] == t["cap"] + t["sort_addend"]
    assert [L.sub_of(b, 10) for b in (0, 40, 41, 80, 81, 160, 161, 100000)] == [4, 4, 8, 8, 16, 16, 16, 16]
    assert [L.ranked_teams(a, 10) for a in (80, 81, 160, 161, 320, 321)] == [(8, 16), (16, 16), (16, 16), (16, 32), (16, 32),
                                                                             (16, 64)]
    assert L.ranked_teams(1000, 10, identity_b=True)[0] == 8


@pytest.mark.parametrize("n", L.SPG_NARROW_NS + (L.SPG_N, L.SPG_N_MAX))
def test_bucket_function_is_monotone_and_below_nbk(n):
    t = L.spg_thresholds()
    cols = np.arange(n) if n <= 1000 else np.unique(np.concatenate([np.arange(1000), n - 1 - np.arange(1000),
                                                                     np.random.default_rng(1).integers(0, n, 5000)]))
    for nbk in (16, 64, t["nbk64"], t["dir_nbk"]):
        assert L.bucket_mul(nbk, n) <= 0xFFFFFFFF
        b = L.bucket_of(cols, nbk, n)
        assert (np.diff(b.astype(np.int64)) >= 0).all() and int(b.max()) < nbk, (n, nbk)


def _rung_rows(f):
    return np.array([f.row_of[g] for g in f.rungs]), list(f.rungs)


@pytest.mark.parametrize("fam", SPG_FAMILIES, ids=SPG_IDS)
def test_family_holds_every_rung_where_it_is_meant_to_be(fam):
    sub, aclass = fam
    t = L.spg_thresholds()
    f = L.spg_family(sub, aclass)
    a1 = t["sort_rounds"] * (t["sort_wave"] // sub)
    # the matrix-wide properties
    assert L.sub_of(f.bc.size, f.k) == sub
    avg_a = f.ac.size / f.m
    assert {8: avg_a <= 8, 16: 8 < avg_a <= 16, 32: 16 < avg_a <= 32, 64: avg_a > 32}[aclass], avg_a
    assert L.ranked_teams(f.ac.size, f.m) == {8: (8, 16), 16: (16, 16), 32: (16, 32), 64: (16, 64)}[aclass]
    assert f.m < 8000 and f.bc.min() == 0 and f.bc.max() == f.n - 1
    assert not np.array_equal(np.diff(f.ar), np.sort(np.diff(f.ar)))             # shuffled
    # the rungs the issue names
    names = set(f.rungs)
    for T in t["bin_limits"]:
        for p in (T - 1, T, T + 1):
            assert {f"edge{p}_many", f"edge{p}_few", f"edge{p}_one"} <= names
        assert {f"equal{T}_many", f"equal{T}_few", f"pairs{T}", f"lastslot{T}", f"bucket{T}"} <= names
        assert {f"sum{T - 1}", f"sum{T}", f"sum{T + 1}"} <= names
    a_lens = {len(g.b_lens) for g in f.rungs.values() if all(x == 1 for x in g.b_lens)}
    assert set(range(0, 71)) <= a_lens
    for w in (8, 16, 32, 64, 128, 256, a1):
        assert {w - 1, w, w + 1} <= a_lens, w
    b_lens = {g.b_lens[0] for nm, g in f.rungs.items() if nm.startswith("blen")}
    assert set(range(0, 21)) | {63, 64, 65, sub - 1, sub, sub + 1, 2 * sub + 1} <= b_lens
    for p in (255, 256, 257):
        for d_len in (1, 63, 64, 65):
            assert {f"add{p}_{d_len}_{o}" for o in ("disjoint", "equal", "half")} <= names
        assert f"add{p}_0_disjoint" in names
    assert {f"addend_only{d}" for d in (65, 257, 1025, 4097)} <= names
    # every rung: product count, bin, distinct columns -- from the ARRAYS, by the reference
    plan3 = L.SpgemmPlan(f.ar, f.ac, f.br, f.bc, (f.m, f.k, f.n))
    plan4 = L.SpgemmPlan(f.ar, f.ac, f.br, f.bc, (f.m, f.k, f.n), f.dr, f.dc)
    bins3, sort3, s3 = L.classify(f.ar, f.ac, f.br)
    bins4, sort4, _ = L.classify(f.ar, f.ac, f.br, f.dr)
    assert s3 == sub
    prod = np.bincount(np.repeat(np.arange(f.m), np.diff(f.ar)), weights=np.diff(f.br)[f.ac], minlength=f.m).astype(int)
    distinct3, distinct4 = np.diff(plan3.rowptr), np.diff(plan4.rowptr)
    extra_len = {"last": f.tails["last"], "prev": f.tails["prev"]}
    for nm, g in f.rungs.items():
        i = f.row_of[nm]
        p = g.products + sum(extra_len[e] for e in g.extra)
        assert prod[i] == p and f.ar[i + 1] - f.ar[i] == len(g.b_lens) + len(g.extra), nm
        assert f.dr[i + 1] - f.dr[i] == g.d_len, nm
        assert bins3[i] == L.bin_of(p) and bins4[i] == L.bin_of(p + g.d_len), nm
        if not g.extra:
            want = {"distinct": p, "all_equal": min(p, 1), "pairs": (p + 1) // 2, "last_slot": p, "one_bucket": p}[g.mode]
            assert distinct3[i] == want, nm
            shared = 0 if g.d_mode == "disjoint" else min(g.d_len, want) if g.d_mode == "equal" else min(g.d_len // 2, want)
            assert distinct4[i] == want + g.d_len - shared, nm
    for T in t["bin_limits"]:                                       # the table of the bin half full; the largest ranks
        assert distinct3[f.row_of[f"edge{T}_many"]] == T and distinct3[f.row_of[f"edge{T - 1}_one"]] == T - 1
    for T in t["bin_limits"]:
        assert f.ar[f.row_of[f"sum{T}"] + 1] - f.ar[f.row_of[f"sum{T}"]] + f.rungs[f"sum{T}"].d_len == T
    # sortable rows: exactly the ones built for it -- stated here by NAME, not through classify
    tail_ok = f.tails["last"] == t["sort_pad"] and f.tails["last"] <= sub          # the last row of B: only a whole vector fits
    want3 = {nm for nm in names if nm.startswith(("sort256_", "add255_", "add256_", "add256pairs_"))} | {"sort65", "tail_prev",
                                                                                                         "tail_prev_add"}
    want3 |= {"tail_last", "tail_last_add"} if tail_ok else set()
    got3 = {nm for nm in names if sort3[f.row_of[nm]]}
    assert got3 == want3, (sorted(got3 - want3), sorted(want3 - got3))
    want4 = {nm for nm in want3 if f.rungs[nm].d_len <= t["sort_addend"]}
    if t["bin_limits"][0] // 2 <= a1:                 # 32 A entries x one-entry B rows + 33 addend entries: bin 2 by the addend
        want4.add(f"sum{t['bin_limits'][0] + 1}")
    got4 = {nm for nm in names if sort4[f.row_of[nm]]}
    assert got4 == want4, (sorted(got4 - want4), sorted(want4 - got4))
    assert bins4[f.row_of["add256_64_disjoint"]] == 3 and distinct4[f.row_of["add256_64_disjoint"]] == t["cap_add"]
    # adversarial columns
    for T, b in zip(t["bin_limits"], (1, 2, 3, 4)):
        i = f.row_of[f"lastslot{T}"]
        cols = plan3.colind[plan3.rowptr[i]:plan3.rowptr[i + 1]]
        assert cols.size == T and (L.spg_hash(cols, t["log2hs"][b]) == (1 << t["log2hs"][b]) - 1).all()
        i = f.row_of[f"bucket{T}"]
        cols = plan3.colind[plan3.rowptr[i]:plan3.rowptr[i + 1]]
        assert cols.size == T and all((L.bucket_of(cols, nbk, f.n) == 0).all() for nbk in (16, 64, t["nbk64"], t["dir_nbk"]))
    # add(): the row sums cross every limit
    sums = np.diff(f.ar) + np.diff(f.add_dr)
    for T in t["bin_limits"]:
        assert {T - 1, T, T + 1} <= set(sums.tolist()), T


def test_the_last_row_of_b_has_every_length_across_the_families():
    lens = {L.spg_family(s, a).tails["last"] for s, a in SPG_FAMILIES}
    assert lens == {1, 2, 3, 4, 5}


def test_small_generators_contain_what_they_claim():
    for n in L.SPG_NARROW_NS:
        ar, ac, br, bc, dr, dc, (m, k, nn) = L.spg_narrow(n)
        assert nn == n and bc.min() == 0 and bc.max() == n - 1 and dc.max() < n
        for d in (None, dr):
            assert set(L.classify(ar, ac, br, d)[0].tolist()) == {0, 1, 2, 3, 4, 5}, n
    ar, ac, br, bc, dr, dc, shape = L.spg_narrow(L.SPG_N_MAX, dense=False)
    assert shape[2] == 2 ** 31 - 1 and {0, 2 ** 30, shape[2] - 1} <= set(bc.tolist())
    for d in (None, dr):
        assert set(L.classify(ar, ac, br, d)[0].tolist()) == {0, 1, 2, 3, 4}
    for m in L.SPG_ROW_COUNTS:
        assert L.spg_row_count_matrix(m)[6][0] == m
    for total in (0, 1, 3, 4, 5):
        ar, ac, br, bc, dr, dc, shape = L.spg_tiny_b(total)
        assert bc.size == total and bool(L.is_sortable(ar, ac, br).any()) == (total >= 4)


@pytest.mark.parametrize("fam", SPG_FAMILIES, ids=SPG_IDS)
def test_exact_data_stay_in_the_exact_range(fam):
    f = L.spg_family(*fam)
    plan = L.SpgemmPlan(f.ar, f.ac, f.br, f.bc, (f.m, f.k, f.n), f.dr, f.dc)
    rng = np.random.default_rng(2)
    av, bv, dv = L.exact_spg_values(rng, (f.ac.size, f.bc.size, f.dc.size))
    assert not (av == 0).any() and set(np.abs(bv).tolist()) == {1.0, 2.0}
    for alpha in L.EXACT_FACTORS:
        ref, abssum = plan.values(av, bv, alpha, dv, -2.0)
        L.assert_exact_range(abssum)
        assert abssum.max() * 2 < 2 ** 24 and (ref * 2 == np.round(ref * 2)).all()
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)       # fp32 holds every result exactly


def _oracle_case(arrays, vt_np, rng):
    from oracle import oracle
    ar, ac, br, bc, dr, dc, (m, k, n) = arrays
    av, bv, dv = [x.astype(vt_np) for x in L.exact_spg_values(rng, (ac.size, bc.size, dc.size))]
    a, b, d = (av, ar, ac, (m, k)), (bv, br, bc, (k, n)), (dv, dr, dc, (m, n))
    rp, ci, v, _, _ = L.spgemm_reference(a, b, -2.0)
    nnz, _ = oracle.spgemm_symbolic((m, k), ar, ac, (k, n), br, bc)
    o_rp, o_ci, o_v = oracle.spgemm_numeric((m, k), ar, ac, av, (k, n), br, bc, bv, capacity=nnz, scale_a=-2.0)
    assert nnz == ci.size and np.array_equal(o_rp, rp) and np.array_equal(o_ci, ci) and np.array_equal(o_v, v.astype(vt_np))
    rp, ci, v, _, _ = L.spgemm_reference(a, b, 0.5, d, -2.0)
    nnz, _ = oracle.spgemm_symbolic_d((m, k), ar, ac, (k, n), br, bc, (m, n), dr, dc)
    o_rp, o_ci, o_v = oracle.spgemm_numeric_d((m, k), ar, ac, av, (k, n), br, bc, bv, (m, n), dr, dc, dv, nnz, alpha=0.5, beta=-2.0)
    assert nnz == ci.size and np.array_equal(o_rp, rp) and np.array_equal(o_ci, ci) and np.array_equal(o_v, v.astype(vt_np))
    return a, d


@pytest.mark.parametrize("fam", SPG_FAMILIES, ids=SPG_IDS)
def test_reference_equals_the_cpu_oracle_on_a_family(fam):
    """The oracle's accumulators are dense in n, so the family is rebuilt at n = 10^6 (its last-slot rungs then hold as many
    colliding columns as lie below that n); structure exactly, exact data bit for bit, fp32 and fp64; add() with B = identity."""
    from oracle import oracle
    f = L.spg_family(*fam, n=1_000_000)
    rng = np.random.default_rng(4)
    for vt_np in (np.float32, np.float64):
        _oracle_case((f.ar, f.ac, f.br, f.bc, f.dr, f.dc, (f.m, f.k, f.n)), vt_np, rng)
        av, dv = [x.astype(vt_np) for x in L.exact_spg_values(rng, (f.ac.size, f.add_dc.size))]
        rp, ci, v, _, _ = L.spgemm_reference((av, f.ar, f.ac, (f.m, f.n)), None, -2.0, (dv, f.add_dr, f.add_dc, (f.m, f.n)), 0.5)
        o_rp, o_ci, o_v = oracle.add((f.m, f.n), f.ar, f.ac, av, (f.m, f.n), f.add_dr, f.add_dc, dv, scale_a=-2.0, scale_b=0.5)
        assert np.array_equal(o_rp, rp) and np.array_equal(o_ci, ci) and np.array_equal(o_v, v.astype(vt_np))


@pytest.mark.parametrize("n", L.SPG_NARROW_NS)
def test_reference_equals_the_cpu_oracle_on_a_narrow_matrix(n):
    _oracle_case(L.spg_narrow(n), np.float64, np.random.default_rng(n))


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("vt", ["f32", "f64"])
def test_spgemm_checkers_pass_the_reference_and_fail_every_mutation(vt, exact):
    f = L.spg_family(8, 32)
    plan = L.SpgemmPlan(f.ar, f.ac, f.br, f.bc, (f.m, f.k, f.n), f.dr, f.dc)
    rng = np.random.default_rng(9)
    sizes = (f.ac.size, f.bc.size, f.dc.size)
    av, bv, dv = L.exact_spg_values(rng, sizes) if exact else [_wide(_cast(vt, L.random_real(rng, s))) for s in sizes]
    alpha, beta = 0.5, -2.0

    def check(values):
        out = _cast(vt, values).numpy()                                # the output type holds the result rounded once
        if exact:
            L.check_spg_exact(vt, out, ref)
        else:
            L.check_spg_random(vt, out, ref, abssum, plan.terms)

    ref, abssum = plan.values(av, bv, alpha, dv, beta)
    check(ref)                                                        # the float64 reference, rounded to the type, passes
    L.check_structure(plan.rowptr, plan.colind, plan)
    terms = plan.term_values(av, bv, alpha, dv, beta)
    row = f.row_of["edge257_few"]                                     # entries that sum ONE product each ...
    row_eq = f.row_of["equal4096_many"]                               # ... and one that sums 4096
    # (RANDOM fp32: one product of 4096 is about as large as the rounding the bound must allow for -- which is why the ladder
    # has the EXACT data; there the entry of 4096 terms is checked too)
    for r in ((row, row_eq) if exact or vt == "f64" else (row,)):
        e = plan.rowptr[r]
        t = int(np.flatnonzero(plan.inv == e)[0])
        for factor, name in ((0.0, "dropped"), (2.0, "doubled")):
            bad = ref.copy()
            bad[e] += (factor - 1.0) * terms[t]
            with pytest.raises(AssertionError):
                check(bad)
    e = plan.rowptr[row]
    bad = ref.copy()
    bad[e], bad[e + 1] = ref[e] + terms[np.flatnonzero(plan.inv == e + 1)[0]], 0.0   # a value lands on the neighbouring entry
    with pytest.raises(AssertionError):
        check(bad)
    cols = plan.colind.copy()
    cols[[e, e + 1]] = cols[[e + 1, e]]                               # two columns of a row swapped
    with pytest.raises(AssertionError):
        L.check_structure(plan.rowptr, cols, plan)
    rp = plan.rowptr.copy()
    rp[row + 1] += 1                                                  # one row offset off by one
    with pytest.raises(AssertionError):
        L.check_structure(rp, plan.colind, plan)
    nan = ref.copy()
    nan[-1] = np.nan                                                  # an entry never written
    with pytest.raises(AssertionError):
        check(nan)
