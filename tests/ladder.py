"""Deterministic ladders for the GPU kernels' tails, and the checkers that go with them (tests/test_gpu_ladders.py runs them on
the device, tests/test_ladders_cpu.py proves on the host that generators and checkers do what they claim).

A kernel that is wrong at ONE row length or ONE column count passes tests that sample sizes.  The ladders walk every size:

  row lengths (SpMV)   every length 0 ... 300; p - 1, p, p + 1 for every power of two p up to 2^17; T - 1, T, T + 1 and
                       2T - 1, 2T, 2T + 1 for every threshold T the kernels branch on.  The thresholds are READ from the
                       sources (thresholds()): the row-block windows of the real, complex and 16-bit kernels, the entries per
                       part of the SpMM long-row kernels, the wave and the SpMM columns per pass; the lanes-per-row steps are the
                       powers of two up to the wave.  The GPU tests assert that the window a plan reports is one of them.
                       Value-free SLICED tiles hold a window of the caller's values per bin in LDS: their ladder runs up to
                       that window's capacity (value_free_window_cap, read from the source), with cap - 1 and cap as rungs and
                       cap + 1 as the asserted fall-back; rows beyond it cannot be value-free.
  column counts (SpMM) every n in 1 ... 160 and {191, 192, 255, 256, 257, 300, 511, 512, 513}; the cap on the parts of a long row
                       is reached by one row of more than 64 * 4096 entries (spmm_capped_parts_matrix).

Two data sets per case.  RANDOM: values and x in (-1, 1), checked with the existing bound of the value type (real:
util.assert_parity with row_len; complex: check_complex; 16-bit: check_lowp -- the latter two moved here from
test_gpu_complex.py / test_gpu_lowp.py unchanged).  EXACT: values in {-1, 0, 1}, x in {-2 ... 2} (real and imaginary parts
alike): every product and every partial sum, in ANY order of summation, is an integer below 2^24 in magnitude because the sum
of |a||x| over the row is (exact_spmv_data asserts it, and asserts the sequential partial sums too; below 2^11 for f16 results,
so that they are integers f16 holds exactly) -- so the result must equal the float64 sum rounded once to the output type,
bit for bit, whatever the kernel's summation order.  A dropped or doubled entry changes an integer: no tolerance hides it.
"""
import os
import re

import numpy as np
import scipy.sparse as sps
import torch

import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spblas-reference_amd", "csrc")

SPMV_COLS = 2000
MAX_POW = 17
SPMM_NS = list(range(1, 161)) + [191, 192, 255, 256, 257, 300, 511, 512, 513]

# ------------------------------------------------------------------------------------------------------------ thresholds


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _two(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: the source no longer has the expected form; update tests/ladder.py"
    return [int(g) for g in m.groups()]


def thresholds():
    """{name: value} of every length / width the kernels branch on, parsed from the sources."""
    spmv, cplx, lowp, spmm = _src("spmv.hip"), _src("complex.hip"), _src("lowp.hip"), _src("spmm.hip")
    t = {}
    t["window_f32"], t["window_f64"] = _two(
        r"struct window_of \{.*?value = sizeof\(T\) == 4 \? (\d+) : (\d+);", spmv.replace("\n", " "), "window_of")
    t["window_c64"], t["window_c128"] = _two(
        r"struct cwindow_of \{.*?value = sizeof\(R\) == 4 \? (\d+) : (\d+);", cplx.replace("\n", " "), "cwindow_of")
    t["window_lowp"], = _two(r"constexpr int LOWP_WIN = (\d+);", lowp, "LOWP_WIN")
    t["spmm_part_entries"], _ = spmm_parts_rule()
    t["spmm_cols_per_pass"], = _two(r"const int cpp = n < (\d+) \? \(int\) n : \1;", spmm, "SpMM columns per pass")
    t["wave"] = 64
    return t


def spmm_parts_rule():
    """(entries per part, most parts per row) of the SpMM long-row kernels: parts = ceil(max_row_len / entries), capped.  The
    cap is a COUNT, not a row length: it is reached by a row of more than entries * cap entries (spmm_capped_parts_matrix)."""
    return _two(r"parts = cdiv\(pl->max_row_len, (\d+)\);\s*parts = parts < 1 \? 1 : \(parts > (\d+) \?", _src("spmm.hip"),
                "SpMM long-row parts")


def lanes_per_row_steps():
    """pick_lpr of spmv.hip / complex.hip / lowp.hip: lanes per row double from 2 to the wave while 1.5 * lanes < the mean row
    length; the row-block kernels' phase 2 doubles from 1.  Every step is a power of two up to 64."""
    return [1 << k for k in range(7)]


def row_lengths():
    """The sorted set of row lengths of the SpMV ladder (see the module docstring)."""
    s = set(range(0, 301))
    for k in range(MAX_POW + 1):
        s.update((max((1 << k) - 1, 0), 1 << k, (1 << k) + 1))
    for t in list(thresholds().values()) + lanes_per_row_steps():
        for base in (t, 2 * t):
            s.update((base - 1, base, base + 1))
    return np.array(sorted(s), dtype=np.int64)


def value_free_window_cap(itemsize, rows_per_bin=1):
    """Entries the LDS window of one bin of a VALUE-FREE SLICED plan can hold -- the one length pb_reduce_vf really branches
    on.  plan_build accepts a bin grid when the widest bin spans at most cap = LDS elements - waves * (rows per bin + 64) - 16
    entries (and fewer than 65 536, which no LDS size reaches: the largest cap is below 41 K); the constants are read from
    spmv_sliced.hip.  With one row per bin (SPBLAS_GFX950_PB_VF_ROWS=1) the span of a bin is the length of its row, so `cap`
    is the longest row value-free tiles take and cap + 1 the shortest they refuse (the plan then falls back to the copying
    form).  The GPU tests pin this number against the library from both sides."""
    src = _src("spmv_sliced.hip")
    kib, minus = _two(r"constexpr int VF_LDS = (\d+) \* 1024 - (\d+);", src, "VF_LDS")
    waves, = _two(r'env_int\("SPBLAS_GFX950_PB_VF_WAVES", (\d+)\)', src, "value-free waves")
    slack, shift = _two(r"cap = \(int64_t\) vf_elems - \(int64_t\) NWv \* \(hh \+ (\d+)\) - (\d+);", src, "value-free window cap")
    return (kib * 1024 - minus) // itemsize - waves * (rows_per_bin + slack) - shift


def value_free_row_lengths(itemsize):
    """The rungs a VALUE-FREE SLICED plan with one row per bin takes: every rung of row_lengths() up to the window's capacity,
    and cap - 1 and cap themselves.  Longer rows cannot fit the window; for them the fall-back is asserted instead."""
    cap = value_free_window_cap(itemsize)
    lens = row_lengths()
    return np.array(sorted(set(lens[lens <= cap].tolist()) | {cap - 1, cap}), dtype=np.int64)


def short_row_lengths():
    """The rungs up to the fp32 row-block window + 1: the ladder for value-free bins of SEVERAL rows (whose span is a sum of
    row lengths, so the long rungs do not fit beside their neighbours)."""
    lens = row_lengths()
    return lens[lens <= thresholds()["window_f32"] + 1]


# ------------------------------------------------------------------------------------------------------------ SpMV ladder
def spmv_ladder(seed=20, lengths=None):
    """(rowptr int64, colind int32, (m, n)): one row per length of row_lengths() (or of `lengths`), rows in shuffled order,
    columns random in [0, SPMV_COLS) with repeats allowed and unsorted within rows."""
    rng = np.random.default_rng(seed)
    lens = rng.permutation(row_lengths() if lengths is None else lengths)
    rowptr = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    colind = rng.integers(0, SPMV_COLS, int(rowptr[-1])).astype(np.int32)
    return rowptr, colind, (int(lens.size), SPMV_COLS)


def random_real(rng, size):
    """float64 values in (-1, 1); the tests cast them to the value type."""
    return rng.uniform(-1, 1, size)


def random_complex(rng, size):
    return rng.uniform(-1, 1, size) + 1j * rng.uniform(-1, 1, size)


def _ints(rng, size, lim, cplx):
    v = rng.integers(-lim, lim + 1, size).astype(np.float64)
    return v + 1j * rng.integers(-lim, lim + 1, size).astype(np.float64) if cplx else v


def max_partial_sum(rowptr, colind, values, x):
    """Largest |sequential partial sum| over all rows (real and imaginary parts separately for complex data), and the
    largest sum of |a||x| over a row: the second bounds every partial sum in every order of summation."""
    prod = values * x[colind]
    parts = (prod.real, prod.imag) if np.iscomplexobj(prod) else (prod,)
    seq = 0.0
    starts = rowptr[:-1][np.diff(rowptr) > 0]
    for p in parts:
        c = np.cumsum(p)
        base = np.concatenate([[0.0], c])[rowptr[:-1]]          # prefix before each row
        row_of = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
        seq = max(seq, float(np.abs(c - base[row_of]).max()) if c.size else 0.0)
    mag = np.abs(values.real) + np.abs(values.imag) if np.iscomplexobj(values) else np.abs(values)
    xm = np.abs(x.real) + np.abs(x.imag) if np.iscomplexobj(x) else np.abs(x)
    anyorder = np.add.reduceat(mag * xm[colind], starts).max() if starts.size else 0.0
    return seq, float(anyorder)


def exact_spmv_data(rowptr, colind, n, cplx=False, f16=False, seed=5):
    """(values, x) of integers: values in {-1, 0, 1}, x in {-2 ... 2}.  Asserts that every partial sum in any order stays
    below 2^24 (exact in fp32, the narrowest accumulation type), and -- f16: the result is to be finite and exactly an
    integer f16 holds -- that the sequential partial sums stay below 2^11; the value set of x is shrunk (never the ladder)
    until they do."""
    rng = np.random.default_rng(seed)
    for xlim in (2, 1):
        values, x = _ints(rng, colind.size, 1, cplx), _ints(rng, n, xlim, cplx)
        seq, anyorder = max_partial_sum(rowptr, colind, values, x)
        if anyorder < 2 ** 24 and (not f16 or seq < 2 ** 11):
            return values, x
    raise AssertionError(f"no exact data set: partial sums reach {seq}, sum |a||x| {anyorder}")


def spmv_reference(rowptr, colind, values, x, shape, conj_a=False, conj_x=False):
    """(float64 / complex128 product, sum |a||x| per row) from the CSR arrays (scipy), never through the library."""
    wide = np.complex128 if np.iscomplexobj(values) or np.iscomplexobj(x) else np.float64
    v, xx = values.astype(wide), x.astype(wide)
    A = sps.csr_matrix((np.conj(v) if conj_a else v, colind, rowptr), shape=shape)
    Aabs = sps.csr_matrix((np.abs(v), colind, rowptr), shape=shape)
    return A @ (np.conj(xx) if conj_x else xx), Aabs @ np.abs(xx)


# ------------------------------------------------------------------------------------------------------------ SpMM ladder
SPMM_SHAPE = (700, 900)
BAND_ROWS = (256, 384)      # a block of rows whose entries lie in a narrow band: qualifies for the panel / band path in f32


def spmm_matrix(seed=31):
    """(rowptr int64, colind int32, shape): about 700 x 900 -- every 9th row empty, rows of 1 ... 40 entries, three rows above
    every plan's window (2 500, 5 000 and 9 000 entries: the last one takes more than one part of spmm_part_entries ...
    and more than two), and rows BAND_ROWS with 24 entries each inside a +-20 column band around the diagonal."""
    rng = np.random.default_rng(seed)
    m, k = SPMM_SHAPE
    lens = 1 + (np.arange(m) * 7) % 40
    lens[::9] = 0
    lens[BAND_ROWS[0]:BAND_ROWS[1]] = 24
    for r, length in ((5, 2500), (444, 5000), (698, 9000)):
        lens[r] = length
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    colind = rng.integers(0, k, int(rowptr[-1])).astype(np.int32)
    for r in range(*BAND_ROWS):
        colind[rowptr[r]:rowptr[r + 1]] = np.clip(r + rng.integers(-20, 21, 24), 0, k - 1)
    return rowptr, colind, (m, k)


def spmm_capped_parts_matrix(seed=37):
    """(rowptr, colind, shape) of a small matrix (64 x 900: rows of 0 ... 40 entries) with ONE row of more than entries * cap
    entries of spmm_parts_rule() (repeated columns, necessarily): the only way to reach the capped branch of the parts."""
    rng = np.random.default_rng(seed)
    per, cap = spmm_parts_rule()
    m, k = 64, SPMM_SHAPE[1]
    lens = (np.arange(m) * 5) % 41
    lens[29] = per * cap + 857
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    return rowptr, rng.integers(0, k, int(rowptr[-1])).astype(np.int32), (m, k)


def spmm_reference(rowptr, colind, values, B, shape, conj_a=False, conj_b=False):
    wide = np.complex128 if np.iscomplexobj(values) or np.iscomplexobj(B) else np.float64
    v, BB = values.astype(wide), B.astype(wide)
    A = sps.csr_matrix((np.conj(v) if conj_a else v, colind, rowptr), shape=shape)
    Aabs = sps.csr_matrix((np.abs(v), colind, rowptr), shape=shape)
    return A @ (np.conj(BB) if conj_b else BB), Aabs @ np.abs(BB)


def exact_spmm_data(rowptr, colind, shape, nmax, cplx=False, f16=False, seed=6):
    """Integer values in {-1, 0, 1} and B in {-2 ... 2} (k x nmax; the tests take its first n columns), with the same
    guarantees as exact_spmv_data for every column of B."""
    rng = np.random.default_rng(seed)
    for blim in (2, 1):
        values, B = _ints(rng, colind.size, 1, cplx), _ints(rng, (shape[1], nmax), blim, cplx)
        mag = np.abs(values.real) + np.abs(values.imag) if cplx else np.abs(values)
        Bm = np.abs(B.real) + np.abs(B.imag) if cplx else np.abs(B)
        anyorder = (sps.csr_matrix((mag, colind, rowptr), shape=shape) @ Bm).max()
        seq = max(max_partial_sum(rowptr, colind, values, B[:, j])[0] for j in range(0, nmax, max(1, nmax // 16)))
        if anyorder < 2 ** 24 and (not f16 or seq < 2 ** 11):
            return values, B
    raise AssertionError(f"no exact SpMM data set: partial sums reach {seq}, sum |a||b| {anyorder}")


SENTINEL = {torch.float32: -7.25, torch.float64: -7.25, torch.float16: -7.25, torch.bfloat16: -7.25,
            torch.complex64: complex(-7.25, 3.5), torch.complex128: complex(-7.25, 3.5)}
LAYOUTS = ["right", "right_ld+1", "right_ld+2", "right_ld+4", "left", "left_ld+1"]
SHIFTS = [(0, 0), (1, 0), (0, 1), (2, 0), (0, 2), (1, 1), (2, 2), (1, 2), (2, 1)]


def dense_window(rows, cols, layout, shift, dtype, device, init=None):
    """(store, view, mask): a 1-D store filled with the sentinel; `view` the rows x cols matrix of the given layout whose
    first element lies `shift` elements into the store (so its base pointer is misaligned by that much) and whose leading
    dimension is cols (+ pad) or rows (+ pad); `mask` marks the store's elements that belong to the view.  Everything else
    is padding the library must never write."""
    pad = int(layout.split("+")[1]) if "+" in layout else 0
    left = layout.startswith("left")
    ld = (rows if left else cols) + pad
    outer = cols if left else rows
    store = torch.full((shift + max(outer, 1) * max(ld, 1) + 8,), 0.0, dtype=dtype, device=device)
    store.fill_(SENTINEL[dtype])
    if left:
        view = torch.as_strided(store, (rows, cols), (1, ld), shift)
    else:
        view = torch.as_strided(store, (rows, cols), (ld, 1), shift)
    mask = torch.zeros(store.shape, dtype=torch.bool, device=device)
    torch.as_strided(mask, (rows, cols), view.stride(), shift).fill_(True)
    if init is not None:
        view.copy_(init)
    return store, view, mask


def bits(t):
    """The tensor's bytes as integers (bitwise comparisons)."""
    t = t.contiguous()
    if t.dtype.is_complex:
        t = torch.view_as_real(t)
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def padding_untouched_t(store, mask, dtype):
    """0-d bool tensor on the store's device (no host synchronisation): every element of the store outside the view still
    holds the sentinel, bit for bit."""
    want = torch.full_like(store, SENTINEL[dtype])
    same = bits(store) == bits(want)
    if dtype.is_complex:
        same = same.all(dim=1)
    return (same | mask).all()


def padding_untouched(store, mask, dtype):
    return bool(padding_untouched_t(store, mask, dtype))


# ------------------------------------------------------------------------------------------------------------ checkers
# complex: moved from tests/test_gpu_complex.py (bound unchanged)
CEPS = {np.complex64: float(np.finfo(np.float32).eps), np.complex128: float(np.finfo(np.float64).eps)}


def check_complex(y, y_ref, absrow, dtype, row_len, what=""):
    """Norm-wise bound per element (util.assert_parity's form, on the complex modulus): the error of a k-entry complex dot
    product in the value type is at most ~(k + 2) * 2 eps * sum |a||x|."""
    eps = CEPS[dtype]
    k = np.maximum(np.asarray(row_len, dtype=np.float64), 16.0)
    if y_ref.ndim == 2 and k.ndim == 1:
        k = k[:, None]
    err = np.abs(y.astype(np.complex128) - y_ref)
    bound = 4.0 * k * eps * absrow + 1e-30
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {bad.sum()} entries off; worst ratio {(err / bound).max():.3g}"


# 16-bit: moved from tests/test_gpu_lowp.py (bound unchanged)
MANT = {torch.float16: 10, torch.bfloat16: 7}   # stored mantissa bits
EMIN = {torch.float16: -14, torch.bfloat16: -126}


def half_ulp(v, dt):
    e = torch.floor(torch.log2(v.clamp(min=1e-300))).clamp(min=EMIN[dt])
    return 0.5 * torch.exp2(e - MANT[dt])


def check_lowp(y, ref, absrow, row_len, dt, what=""):
    """y: 16-bit device tensor; ref / absrow: float64 (numpy or torch) of y's shape; row_len: entries per row."""
    yd = y.double()
    ref = torch.as_tensor(ref, dtype=torch.float64).to(yd.device)
    absrow = torch.as_tensor(absrow, dtype=torch.float64).to(yd.device)
    k = torch.as_tensor(np.asarray(row_len, dtype=np.float64)).to(yd.device)
    if ref.dim() == 2 and k.dim() == 1:
        k = k[:, None]
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(yd), nan), f"{what}: NaN positions differ"
    inf = torch.isinf(ref)
    assert torch.equal(yd[inf], ref[inf]), f"{what}: inf entries differ"
    acc = (k + 2.0) * 2.0 ** -24 * absrow
    bound = half_ulp(ref.abs() + acc, dt) + acc
    bad = ~nan & ~inf & ~((yd - ref).abs() <= bound)
    if bool(bad.any()):
        idx = bad.nonzero()[:5].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound, first at {idx}: "
                             f"{[(yd[tuple(i)].item(), ref[tuple(i)].item(), bound[tuple(i)].item()) for i in idx]}")


def bits_equal(y, ref64, dt):
    """y (16-bit) equals ref64 rounded to dt bit for bit (+0 / -0 taken as one value)."""
    r = torch.as_tensor(ref64, dtype=torch.float64).to(y.device).to(dt)
    yb, rb = y.view(torch.int16), r.view(torch.int16)
    yb = torch.where(y == 0, torch.zeros_like(yb), yb)
    rb = torch.where(r == 0, torch.zeros_like(rb), rb)
    return torch.equal(yb, rb)


TORCH_OF = {"f32": torch.float32, "f64": torch.float64, "c64": torch.complex64, "c128": torch.complex128,
            "f16": torch.float16, "bf16": torch.bfloat16}
NUMPY_OF = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}


def cast(vt, a):
    """float64 / complex128 numpy -> torch tensor (host) of the value type `vt`: one rounding."""
    return torch.as_tensor(np.asarray(a)).to(TORCH_OF[vt])


def wide(t):
    """A tensor of any value type as float64 / complex128 numpy: the inputs exactly as the kernel is given them."""
    return t.detach().cpu().to(torch.complex128 if t.dtype.is_complex else torch.float64).numpy()


def check_random(vt, y, ref, absrow, row_len, what=""):
    """The existing bound of the value type `vt` (a key of TORCH_OF); y: torch tensor (any device) of that type."""
    if vt in ("f16", "bf16"):
        return check_lowp(y, ref, absrow, row_len, TORCH_OF[vt], what)
    yh = y.cpu().numpy()
    if vt in ("c64", "c128"):
        return check_complex(yh, ref, absrow, NUMPY_OF[vt], row_len, what)
    return util.assert_parity(yh, ref, absrow, NUMPY_OF[vt], row_len=row_len, what=what)


def check_exact(vt, y, ref, what=""):
    """y equals the float64 / complex128 reference rounded ONCE to the output type, bit for bit (+0 and -0 are one value: a
    sum of integers that cancels has no sign to get wrong).  A NaN (an element never written) fails."""
    dt = TORCH_OF[vt]
    want = torch.as_tensor(np.asarray(ref)).to(torch.complex128 if dt.is_complex else torch.float64).to(dt)
    got = y.detach().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    gb, wb = bits(got), bits(want)
    gr = torch.view_as_real(got.contiguous()) if dt.is_complex else got.contiguous()
    wr = torch.view_as_real(want.contiguous()) if dt.is_complex else want.contiguous()
    gb = torch.where(gr == 0, torch.zeros_like(gb), gb)
    wb = torch.where(wr == 0, torch.zeros_like(wb), wb)
    bad = gb != wb
    if bool(bad.any()):
        idx = bad.nonzero()[:5].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ from the exact result, first at {idx}: "
                             f"{[(gr[tuple(i)].item(), wr[tuple(i)].item()) for i in idx]}")
