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

SpGEMM / add (csrc/spgemm.hip; the second half of this module, run by tests/test_gpu_spgemm_ladders.py).  A RUNG is one row of A
with B rows of its own: (lengths of the B rows it selects, how the products' columns coincide -- distinct, all equal, pairs,
all hashing to the last slot of the bin's table, all in bucket 0 of the rank sorts --, length of the addend's row and whether
its columns are disjoint from, among, or half shared with the products').  spg_rungs(sub) lists them: T - 1, T, T + 1 products
for every bin limit T in three shapes; A rows of 0 ... 70 entries and w - 1, w, w + 1 for every team width w; B rows of
0 ... 20, 63 ... 65, sub - 1 ... sub + 1, 2 sub + 1 entries; every condition of the sortable rule met and missed by one; addend rows
of 0 / 1 / 63 / 64 / 65 entries on 255 / 256 / 257 products (256 + 64: the 320th slot); addend rows that decide the bin alone;
rows that select the last rows of B's arrays.  `sub` (lanes per B row) and the team widths of the fills by rank are properties
of the whole matrix, so spg_family(sub, aclass) packs the ~250 rungs into one matrix triple whose padding rows set them:
sub in {4, 8, 16} x A's mean row length <= 8, <= 16, <= 32, > 32 -- twelve families of 570 ... 7 100 rows of A, 43 000 ... 54 000
rows of B with 0.11 ... 0.76 M entries, 0.11 ... 0.71 M products, C 40 M columns wide (4 096 columns that hash to the last of
8 192 slots lie below 3.4e7); the last row of B has 1 ... 5 entries across the families.  Narrow C (n = 1 ... 257, rows in every
bin), the widest n the C ABI takes (2^31 - 1, no dense-bin row), row counts around the strides of the symbolic passes and B
with 0 ... 5 entries have small generators of their own.  The constants come from the source (spg_thresholds) and the binning
pass is restated in classify().  EXACT data: values from {-2, -1, 1, 2}, factors from {1, -2, 0.5}, sum of |terms| per entry
below 2^23 (asserted): every partial sum is a multiple of 1/2 that fp32 holds.  RANDOM data: per-entry bound
max(util.TOL, (t + 2) / 2 eps) sum |terms| with t the terms of that entry.  Reference: SpgemmPlan (numpy only).
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
    """pick_lpr of spmv.hip (the one rule of every value type's vector kernels): lanes per row double from 2 to the wave while
    1.5 * lanes < the mean row length; the row-block kernels' phase 2 doubles from 1.  Every step is a power of two up to 64."""
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


# =================================================================================================== SpGEMM / add ladder
SPG_N = 40_000_000          # columns of C in the families: wide enough for 4096 columns that hash to the last slot of bin 4
SPG_SUBS = (4, 8, 16)
SPG_ACLASSES = (8, 16, 32, 64)     # A's mean row length: <= 8, <= 16, <= 32, > 32 (the steps of launch_ranked)
SPG_NARROW_NS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
SPG_ROW_COUNTS = (0, 1, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
SPG_N_MAX = 2 ** 31 - 1
EXACT_VALUES = np.array([-2.0, -1.0, 1.0, 2.0])
EXACT_FACTORS = (1.0, -2.0, 0.5)
_HASH_MUL = 0x9E3779B1


def spg_thresholds():
    """Every constant csrc/spgemm.hip branches on, parsed from the source (a pattern that no longer matches fails with
    "update tests/ladder.py")."""
    src = _src("spgemm.hip")
    flat = re.sub(r"\s+", " ", src)
    t = {}
    t["bin_limits"] = _two(r"if \(ub == 0\) return 0; if \(ub <= (\d+)\) return 1; if \(ub <= (\d+)\) return 2; "
                           r"if \(ub <= (\d+)\) return 3; if \(ub <= (\d+)\) return 4; return 5;", flat, "spg_bin_of")
    log2hs, tpr = {}, {}
    for b in (1, 3, 4):
        log2hs[b], tpr[b] = _two(r"launch_hash<T, (\d+), (\d+), NUMERIC>\(s, st, %d," % b, flat, f"launch_hash of bin {b}")
    log2hs[2], tpr[2], _ = _two(r"launch_hash<T, (\d+), NUMERIC \? (\d+) : (\d+), NUMERIC>\(s, st, 2,", flat,
                                "launch_hash of bin 2")
    t["log2hs"], t["team"] = log2hs, tpr
    (t["sort_rounds"], t["sort_wave"], t["sort_a_max"], t["sort_products"], t["sort_addend"]) = _two(
        r"p1 - p0 <= (\d+) \* \((\d+) / sub\) && p1 - p0 <= (\d+) && ub_prod <= (\d+) && d_len <= (\d+)\)", flat,
        "the sortable rule of spg_bound_kernel")
    t["sort_pad"], = _two(r"bad \|= \(int\) \(dd\.y > sub\) \| \(int\) \(\(int64_t\) dd\.x \+ \(\(dd\.y \+ (\d+)\) & ~\1\) > b_nnz\);",
                          flat, "the padded-range rule of spg_bound_kernel")
    t["sort_pad"] += 1
    t["sort_b_nnz"], = _two(r"st->r_adesc && b_nnz >= (\d+) &&", flat, "sortable_ok")
    t["cap_add"], t["cap"] = _two(r"constexpr int CAP = ADD \? (\d+) : (\d+);", flat, "CAP of spg_direct_kernel")
    t["nbk64"], = _two(r"#define SPG_NBK64 (\d+)", src, "SPG_NBK64")
    t["dir_nbk"], = _two(r"#define SPG_DIR_NBK (\d+)", src, "SPG_DIR_NBK")
    t["sub_min"], t["sub_max"] = _two(r"st->sub = (\d+); while \(st->sub < 64 && st->sub < avg_b\) st->sub <<= 1; "
                                      r"if \(st->sub > (\d+)\)", flat, "the rule for sub")
    t["tpr2_steps"] = _two(r"tpr_env : avg_a <= (\d+)\.0 \? (\d+) : avg_a <= (\d+)\.0 \? (\d+) : (\d+);", flat,
                           "the bin-2 team widths of launch_ranked")
    t["tpr1_steps"] = _two(r"\(st->identity_b \|\| avg_a <= (\d+)\.0\) \? (\d+) : (\d+);", flat,
                           "the bin-1 team widths of launch_ranked")
    t["rank_caps"] = _two(r"prod\[row\] = ub <= (\d+) \? \(int32_t\) ub : 0; prod3\[row\] = ub > \1 && ub <= (\d+) \?", flat,
                          "the rank widths of spg_products_kernel")
    m = re.search(r"\(unsigned\) key \* 0x([0-9A-Fa-f]+)u\) >> \(32 - log2hs\)", src)
    assert m and int(m.group(1), 16) == _HASH_MUL, "spg_hash: the source no longer has the expected form; update tests/ladder.py"
    return t


def bin_of(products):
    """spg_bin_of, vectorised: 0 for no product, then one bin per limit, 5 beyond the last."""
    p = np.asarray(products, dtype=np.int64)
    return np.where(p == 0, 0, 1 + np.searchsorted(np.asarray(spg_thresholds()["bin_limits"]), p, side="left"))


def sub_of(b_nnz, k):
    """Lanes per B row: the power of two from sub_min that reaches B's mean row length, at most sub_max."""
    t = spg_thresholds()
    avg, sub = (b_nnz / k if k > 0 else 0.0), t["sub_min"]
    while sub < 64 and sub < avg:
        sub <<= 1
    return min(sub, t["sub_max"])


def ranked_teams(a_nnz, m, identity_b=False):
    """(team width of bin 1, of bin 2) of the fills by rank (launch_ranked), from A's mean row length."""
    t = spg_thresholds()
    avg = a_nnz / m if m > 0 else 0.0
    s2, s1 = t["tpr2_steps"], t["tpr1_steps"]
    return (s1[1] if identity_b or avg <= s1[0] else s1[2]), (s2[1] if avg <= s2[0] else s2[3] if avg <= s2[2] else s2[4])


def spg_hash(col, log2hs):
    return ((np.asarray(col, dtype=np.uint64) * np.uint64(_HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - log2hs)


def bucket_mul(nbk, n):
    return min((nbk << 32) // max(int(n), 1), 0xFFFFFFFF)


def bucket_of(col, nbk, n):
    """umulhi(col, floor(nbk * 2^32 / n)) with the clamped multiplier (spg_bucket_mul)."""
    return (np.asarray(col, dtype=np.uint64) * np.uint64(bucket_mul(nbk, n))) >> np.uint64(32)


_LAST_SLOT = {}


def last_slot_columns(log2hs, count, n, strict=True):
    """The first `count` columns below n whose spg_hash for a table of 2^log2hs slots is the LAST slot (strict=False: as many
    of them as lie below n)."""
    key = (log2hs, n)
    have = _LAST_SLOT.get(key, (np.zeros(0, np.int64), 0))
    cols, upto = have
    while cols.size < count and upto < n:
        hi = min(upto + (1 << 22), n)
        a = np.arange(upto, hi, dtype=np.int64)
        cols = np.concatenate([cols, a[spg_hash(a, log2hs) == (1 << log2hs) - 1]])
        upto = hi
    _LAST_SLOT[key] = (cols, upto)
    assert cols.size >= count or not strict, f"only {cols.size} of {count} last-slot columns below {n}"
    return cols[:count]


def classify(ar, ac, br, dr=None, identity_b=False, direct=True, adesc=True, direct_add=True):
    """The binning pass of the symbolic call (spg_bound_kernel) restated on the host: (bin 0 .. 5 per row, sortable flag per
    row, sub).  br = None with identity_b: add().  A sortable row is counted in bin 2's range whatever its own bin."""
    t = spg_thresholds()
    ar, ac = np.asarray(ar, dtype=np.int64), np.asarray(ac, dtype=np.int64)
    m = ar.size - 1
    a_len = np.diff(ar)
    row_of = np.repeat(np.arange(m), a_len)
    if identity_b:
        blen, bstart, b_nnz, k = np.ones(ac.size, np.int64), ac, 0, 0
    else:
        br = np.asarray(br, dtype=np.int64)
        blen, bstart, b_nnz, k = np.diff(br)[ac], br[:-1][ac], int(br[-1]), br.size - 1
    sub = sub_of(b_nnz, k)
    prod = np.bincount(row_of, weights=blen, minlength=m).astype(np.int64) if m else np.zeros(0, np.int64)
    d_len = np.diff(np.asarray(dr, dtype=np.int64)) if dr is not None else np.zeros(m, np.int64)
    b = bin_of(prod + d_len)
    pad = t["sort_pad"]
    bad_e = (blen > sub) | (bstart + (blen + pad - 1) // pad * pad > b_nnz)
    bad = np.bincount(row_of, weights=bad_e, minlength=m) > 0 if m else np.zeros(0, bool)
    ok = (direct and not identity_b and adesc and ac.size > 0 and b_nnz >= t["sort_b_nnz"] and (dr is None or direct_add))
    sortable = ((b == 2) | ((b == 3) & (dr is not None))) & ok & ~bad & (a_len <= t["sort_rounds"] * (t["sort_wave"] // sub)) & \
        (a_len <= t["sort_a_max"]) & (prod <= t["sort_products"]) & (d_len <= t["sort_addend"])
    return b, sortable, sub


def is_sortable(ar, ac, br, dr=None, **kw):
    return classify(ar, ac, br, dr, **kw)[1]


def predicted_info(ar, ac, br, dr=None, **kw):
    """What spgemm_state_t.info() must report after the symbolic pass."""
    b, s, sub = classify(ar, ac, br, dr, **kw)
    cnt = np.bincount(np.where(s, 2, b), minlength=6)
    return {"wave_per_row_rows": int(cnt[2]), "direct_rows": int(s.sum()), "lanes_per_b_row": sub,
            "bin1_rows": int(cnt[1]), "bin3_rows": int(cnt[3]), "dense_rows": int(cnt[5]), "bin4_rows": int(cnt[4]),
            "empty_rows": int(cnt[0])}


# ---------------------------------------------------------------------------------------------------------------- rungs
class Rung:
    """One row of A: the lengths of the B rows it selects (each its own), how the products' columns coincide, the addend's row."""

    def __init__(self, name, b_lens, mode="distinct", d_len=0, d_mode="disjoint", extra=()):
        self.name, self.b_lens, self.mode, self.d_len, self.d_mode, self.extra = name, list(b_lens), mode, d_len, d_mode, extra

    @property
    def products(self):
        return int(sum(self.b_lens))


def _split(p, rows):
    """p products over `rows` B rows, as evenly as possible (the first rows take the remainder)."""
    rows = max(1, min(rows, p)) if p else 0
    return [p // rows + (1 if i < p % rows else 0) for i in range(rows)]


def spg_rungs(sub):
    """The rungs of the module docstring for a matrix whose B rows get `sub` lanes; names are unique."""
    t = spg_thresholds()
    a1 = t["sort_rounds"] * (t["sort_wave"] // sub)       # longest A row of a sortable row
    r = []
    for T in t["bin_limits"]:
        for p in (T - 1, T, T + 1):
            r.append(Rung(f"edge{p}_many", [1] * p))
            r.append(Rung(f"edge{p}_few", _split(p, 4)))
            r.append(Rung(f"edge{p}_one", [p]))
        r.append(Rung(f"equal{T}_many", [1] * T, "all_equal"))
        r.append(Rung(f"equal{T}_few", _split(T, 4), "all_equal"))
        r.append(Rung(f"pairs{T}", _split(T, 8), "pairs"))
        r.append(Rung(f"lastslot{T}", _split(T, 8), "last_slot"))
        r.append(Rung(f"bucket{T}", _split(T, 8), "one_bucket"))
    r.append(Rung("equal6000", _split(6000, 5), "all_equal"))          # dense bin, every product on one column
    widths = sorted({w + o for w in (8, 16, 32, 64, 128, 256, a1) for o in (-1, 0, 1)} | set(range(0, 71)))
    have = {x.name for x in r}
    for L in widths:
        if f"edge{L}_many" not in have:
            r.append(Rung(f"alen{L}", [1] * L))
    for L in sorted(set(range(0, 21)) | {63, 64, 65, sub - 1, sub, sub + 1, 2 * sub + 1}):
        r.append(Rung(f"blen{L}", [L, L, 2]))
        r.append(Rung(f"blen{L}_pairs", [L, L, 2], "pairs"))
    # sortable shapes: one round of loads
    full = [sub] * a1
    for mode in ("distinct", "pairs", "all_equal", "last_slot", "one_bucket"):
        r.append(Rung(f"sort256_{mode}", full, mode))
    r.append(Rung("sort65", _split(65, -(-65 // sub))))
    r.append(Rung("sort64_bin1", _split(64, -(-64 // sub))))
    r.append(Rung("sort_a_plus1", [sub] * (a1 - 1) + [sub - 1, 1]))     # 256 products, an A row one entry too long
    r.append(Rung("sort_b_plus1", [sub + 1] + [sub] * (a1 - 2)))        # one B row one entry too long
    for p in (255, 256, 257):
        lens = [sub] * (a1 - 1) + [sub - 1] if p == 255 else full if p == 256 else full + [1]
        for d_len in (0, 1, 63, 64, 65):
            for d_mode in (("disjoint",) if d_len == 0 else ("disjoint", "equal", "half")):
                r.append(Rung(f"add{p}_{d_len}_{d_mode}", lens, "distinct", d_len, d_mode))
    for d_mode in ("disjoint", "equal", "half"):
        r.append(Rung(f"add256pairs_64_{d_mode}", full, "pairs", 64, d_mode))
    for d_len in (1, 64, 65, 257, 1025, 4097):
        r.append(Rung(f"addend_only{d_len}", [], "distinct", d_len))
    for T in t["bin_limits"]:                                           # add(): len(A_i) + len(D_i) around every limit
        for o in (-1, 0, 1):
            r.append(Rung(f"sum{T + o}", [1] * (T // 2), "distinct", T - T // 2 + o, "half"))
    for tail in ("last", "prev"):                                       # rows that select the B rows at the end of B's arrays
        r.append(Rung(f"tail_{tail}", [sub] * (a1 - 2), "distinct", 0, "disjoint", (tail,)))
        r.append(Rung(f"tail_{tail}_add", [sub] * (a1 - 2), "distinct", 5, "half", (tail,)))
    names = [x.name for x in r]
    assert len(set(names)) == len(names)
    return r


def _distinct(rng, n, count, avoid=None):
    """`count` distinct columns in [0, n), none of `avoid`, in random order."""
    got = np.zeros(0, np.int64)
    assert count <= n - (0 if avoid is None else np.unique(avoid).size)
    while got.size < count:
        c = np.unique(rng.integers(0, n, 2 * (count - got.size) + 8))
        if avoid is not None:
            c = np.setdiff1d(c, avoid)
        got = np.union1d(got, c)
    return rng.permutation(got)[:count]


def _product_columns(rng, rung, n, log2hs):
    p = rung.products
    if rung.mode == "distinct":
        return _distinct(rng, n, p)
    if rung.mode == "all_equal":
        return np.full(p, int(rng.integers(0, n)), np.int64)
    if rung.mode == "pairs":
        d = _distinct(rng, n, (p + 1) // 2)
        return rng.permutation(np.concatenate([d, d])[:p])
    if rung.mode == "last_slot":
        c = last_slot_columns(log2hs[int(bin_of(p))], p, n, strict=n >= SPG_N) if p else np.zeros(0, np.int64)
        return rng.permutation(np.concatenate([c, _distinct(rng, n, p - c.size, avoid=c)]))
    if rung.mode == "one_bucket":
        return rng.permutation(np.arange(p, dtype=np.int64))
    raise ValueError(rung.mode)


def _addend_columns(rng, d_len, d_mode, pcols, n):
    have = np.unique(pcols)
    shared = 0 if d_mode == "disjoint" else min(d_len, have.size) if d_mode == "equal" else min(d_len // 2, have.size)
    own = _distinct(rng, n, d_len - shared, avoid=have)
    return rng.permutation(np.concatenate([rng.permutation(have)[:shared], own]))


class Family:
    pass


_FAMILIES = {}


def spg_family(sub, aclass, seed=41, n=SPG_N):
    """One matrix triple (A m x k, B k x n, D m x n; int32 CSR arrays, structure only) that holds every rung of spg_rungs(sub),
    one row of A each with B rows of its own, plus padding rows that bring B's mean row length into the class of `sub` and
    A's into `aclass`; rows shuffled.  Also D for add() (`add_dr`, `add_dc`: half of each row's columns shared with A's row
    taken as a row of an m x n matrix).  `row_of[name]` is the row of a rung."""
    key = (sub, aclass, seed, n)
    if key in _FAMILIES:
        return _FAMILIES[key]
    t = spg_thresholds()
    rng = np.random.default_rng(seed + 100 * sub + aclass)
    rungs = spg_rungs(sub)
    tails = {"prev": 3, "last": 1 + (SPG_SUBS.index(sub) * len(SPG_ACLASSES) + SPG_ACLASSES.index(aclass)) % 5}
    b_rows, a_rows, d_rows = [], [], []           # lists of column arrays; a_rows: indices of B rows (filled below)
    for g in rungs:
        pcols = _product_columns(rng, g, n, t["log2hs"])
        if g.name == "edge64_few":
            pcols[:2] = (0, n - 1)                # the first and the last column of C are in use
        first = len(b_rows)
        cuts = np.cumsum([0] + g.b_lens)
        b_rows.extend(pcols[cuts[i]:cuts[i + 1]] for i in range(len(g.b_lens)))
        a_rows.append((list(range(first, len(b_rows))), g.extra))
        d_rows.append(_addend_columns(rng, g.d_len, g.d_mode, pcols, n))
    # B's padding rows: bring the mean row length to the middle of the class of `sub`
    lo, hi = {4: (0, 4), 8: (4, 8), 16: (8, 24)}[sub]
    target = (lo + hi) / 2
    rows_b, ent_b = len(b_rows) + 2, sum(len(x) for x in b_rows) + sum(tails.values())
    pad_len = 0 if ent_b / rows_b > target else int(3 * target)
    pad_rows = int(abs(target * rows_b - ent_b) / abs(pad_len - target)) + 64
    pad_first = len(b_rows)
    for i in range(pad_rows):
        L = max(0, pad_len + (i % 5) - 2) if pad_len else (i % 4 if i < 64 else 0)
        b_rows.append(_distinct(rng, n, L))
    n_pad_b = len(b_rows) - pad_first
    tail_index = {}
    for name in ("prev", "last"):                 # the last two rows of B: `last` ends where B's arrays end
        tail_index[name] = len(b_rows)
        b_rows.append(_distinct(rng, n, tails[name]))
    a_idx = [np.array(own + [tail_index[e] for e in extra], np.int64) for own, extra in a_rows]
    names = [g.name for g in rungs]
    # A's padding rows select B's padding rows
    ent_a, rows_a = sum(x.size for x in a_idx), len(a_idx)
    a_lo, a_hi = {8: (2, 8), 16: (8, 16), 32: (16, 32), 64: (32, 96)}[aclass]
    a_target = a_lo + 0.85 * (a_hi - a_lo) if aclass < 64 else 64.0
    a_pad_len = 2 if ent_a / rows_a > a_target else int(2.5 * a_target)
    a_pad_rows = int(abs(a_target * rows_a - ent_a) / abs(a_pad_len - a_target)) + 32
    for i in range(a_pad_rows):
        L = max(0, a_pad_len + (i % 5) - 2)
        a_idx.append(pad_first + rng.integers(0, n_pad_b if pad_len else 64, L))   # (no padding length: only the first 64 hold entries)
        d_rows.append(_distinct(rng, n, i % 4))
        names.append(None)
    perm = rng.permutation(len(a_idx))
    a_idx, d_rows, names = [a_idx[i] for i in perm], [d_rows[i] for i in perm], [names[i] for i in perm]

    def csr(rows):
        rp = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(x) for x in rows], out=rp[1:])
        ci = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        assert rp[-1] < 2 ** 31
        return rp.astype(np.int32), ci.astype(np.int32)

    f = Family()
    f.sub, f.aclass, f.name = sub, aclass, f"sub{sub}_a{aclass}"
    f.ar, f.ac = csr(a_idx)
    f.br, f.bc = csr(b_rows)
    f.dr, f.dc = csr(d_rows)
    f.m, f.k, f.n = len(a_idx), len(b_rows), n
    f.names = names
    f.row_of = {nm: i for i, nm in enumerate(names) if nm is not None}
    f.rungs = {g.name: g for g in rungs}
    f.tails = tails
    # add(): A as an m x n matrix (its columns are below k <= n) plus a second summand that shares half of each row's columns
    add_rows = []
    for i, cols in enumerate(a_idx):
        g = f.rungs.get(names[i])
        d_len = g.d_len if g is not None and g.d_len else i % 7
        add_rows.append(_addend_columns(rng, d_len, "half", cols, n))
    f.add_dr, f.add_dc = csr(add_rows)
    assert f.k <= n
    _FAMILIES[key] = f
    return f


def spg_families():
    return [(s, a) for s in SPG_SUBS for a in SPG_ACLASSES]


# ------------------------------------------------------------------------------------------ narrow, widest, row-count, tiny B
def spg_narrow(n, seed=53, dense=True):
    """(ar, ac, br, bc, dr, dc, (m, k, n)) with C only n columns wide and rows in every bin n admits (the product count has no
    such limit); columns 0 and n - 1 are in every B row of two entries or more.  dense=False: no row beyond the last limit."""
    rng = np.random.default_rng(seed + n % 1000)
    b_lens = [i % 13 for i in range(300)] + [1500] + ([4200] if dense else [])
    k = len(b_lens)
    b_rows = []
    for L in b_lens:
        c = rng.integers(0, n, L)
        if L >= 2:
            c[0], c[-1] = 0, n - 1
        b_rows.append(c)
    if n == SPG_N_MAX and b_rows[1].size:
        b_rows[3][1] = 2 ** 30
    a_lens = [0, 1, 2, 5, 10, 11, 16, 17, 20, 30, 40, 41, 42, 43, 44, 60, 100, 170, 171, 180, 400, 600] * 3
    a_rows = [rng.integers(0, 300, L) for L in a_lens]
    a_rows.append(np.array([300, 5, 7]))                       # 1500 + a few products
    a_rows.append(np.array([300, 300]))                        # 3000
    if dense:
        a_rows.append(np.array([301]))
        a_rows.append(np.array([301, 300, 9]))
    m = len(a_rows)
    d_rows = [np.unique(rng.integers(0, n, (i * 7) % 90)) for i in range(m)]

    def csr(rows):
        rp = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(x) for x in rows], out=rp[1:])
        return rp.astype(np.int32), np.concatenate(rows).astype(np.int32)

    (ar, ac), (br, bc), (dr, dc) = csr(a_rows), csr(b_rows), csr(d_rows)
    return ar, ac, br, bc, dr, dc, (m, k, n)


def spg_row_count_matrix(m, seed=59):
    """Short random rows, m of them: the symbolic passes stride by 32, 1024 and 2048 rows."""
    rng = np.random.default_rng(seed + m)
    k, n = 50, 200
    a_lens, b_lens = rng.integers(0, 7, m), rng.integers(0, 9, k)
    ar = np.concatenate([[0], np.cumsum(a_lens)]).astype(np.int32)
    br = np.concatenate([[0], np.cumsum(b_lens)]).astype(np.int32)
    ac = rng.integers(0, k, int(ar[-1])).astype(np.int32)
    bc = rng.integers(0, n, int(br[-1])).astype(np.int32)
    d_lens = rng.integers(0, 4, m)
    dr = np.concatenate([[0], np.cumsum(d_lens)]).astype(np.int32)
    dc = rng.integers(0, n, int(dr[-1])).astype(np.int32)
    return ar, ac, br, bc, dr, dc, (m, k, n)


def spg_tiny_b(total, seed=61):
    """B with `total` entries in all (0, 1, 3, 4, 5: around the least B the vector loads of the sortable rows accept)."""
    rng = np.random.default_rng(seed + total)
    k, n, m = 6, 5000, 40
    b_lens = np.zeros(k, np.int64)
    b_lens[2], b_lens[4] = min(total, 4), total - min(total, 4)     # (rows that select row 2 alone are sortable if B has a vector)
    br = np.concatenate([[0], np.cumsum(b_lens)]).astype(np.int32)
    bc = rng.permutation(n)[:total].astype(np.int32)
    a_lens = np.array([(i * 29) % 130 for i in range(m)])
    ar = np.concatenate([[0], np.cumsum(a_lens)]).astype(np.int32)
    ac = rng.integers(0, k, int(ar[-1])).astype(np.int32)
    for i in range(0, m, 3):
        ac[ar[i]:ar[i + 1]] = 2
    dr = np.arange(m + 1, dtype=np.int32)
    dc = rng.integers(0, n, m).astype(np.int32)
    return ar, ac, br, bc, dr, dc, (m, k, n)


# ------------------------------------------------------------------------------------------------------------ reference
class SpgemmPlan:
    """The structure of C = alpha A B + beta D worked out once on the host (numpy only -- neither the library nor oracle/):
    every product and every addend entry becomes a key row * n + column; np.unique gives C's structure and the output
    entry of every term.  values() then sums float64 terms per entry.  B = None: the identity (add())."""

    def __init__(self, ar, ac, br, bc, shape, dr=None, dc=None):
        m, k, n = shape
        ar, ac = np.asarray(ar, np.int64), np.asarray(ac, np.int64)
        row_of_a = np.repeat(np.arange(m, dtype=np.int64), np.diff(ar))
        if br is None:
            self.e_of, self.q, cols = np.arange(ac.size), None, ac
        else:
            br, bc = np.asarray(br, np.int64), np.asarray(bc, np.int64)
            blen = np.diff(br)[ac]
            self.e_of = np.repeat(np.arange(ac.size, dtype=np.int64), blen)
            first = np.cumsum(blen) - blen
            self.q = br[:-1][ac][self.e_of] + np.arange(int(blen.sum()), dtype=np.int64) - first[self.e_of]
            cols = bc[self.q]
        keys = row_of_a[self.e_of] * n + cols
        self.n_prod = keys.size
        if dr is not None:
            dr = np.asarray(dr, np.int64)
            keys = np.concatenate([keys, np.repeat(np.arange(m, dtype=np.int64), np.diff(dr)) * n + np.asarray(dc, np.int64)])
        uk, self.inv = np.unique(keys, return_inverse=True)
        self.inv = self.inv.reshape(-1)
        self.nnz = uk.size
        self.colind = (uk % n).astype(np.int32)
        self.rowptr = np.concatenate([[0], np.cumsum(np.bincount(uk // n, minlength=m))]).astype(np.int32) if m else np.zeros(1, np.int32)
        self.terms = np.bincount(self.inv, minlength=self.nnz)
        self.shape = shape

    def term_values(self, av, bv, alpha=1.0, dv=None, beta=1.0):
        av = np.asarray(av, np.float64)
        t = alpha * av[self.e_of] if self.q is None else (alpha * av[self.e_of]) * np.asarray(bv, np.float64)[self.q]
        if dv is not None:
            t = np.concatenate([t, beta * np.asarray(dv, np.float64)])
        return t

    def values(self, av, bv, alpha=1.0, dv=None, beta=1.0):
        """(float64 values of C, sum of |terms| per entry)."""
        t = self.term_values(av, bv, alpha, dv, beta)
        return np.bincount(self.inv, weights=t, minlength=self.nnz), np.bincount(self.inv, weights=np.abs(t), minlength=self.nnz)


def spgemm_reference(a, b, alpha=1.0, d=None, beta=1.0):
    """a, b, d: (values, rowptr, colind, shape) (b = None: identity; d optional).  Returns (rowptr, colind, float64 values,
    sum |terms| per entry, terms per entry)."""
    av, ar, ac, ash = a
    shape = (ash[0], ash[1], ash[1] if b is None else b[3][1])
    plan = SpgemmPlan(ar, ac, None if b is None else b[1], None if b is None else b[2], shape,
                      None if d is None else d[1], None if d is None else d[2])
    v, s = plan.values(av, None if b is None else b[0], alpha, None if d is None else d[0], beta)
    return plan.rowptr, plan.colind, v, s, plan.terms


def exact_spg_values(rng, sizes):
    """One array per size with values from {-2, -1, 1, 2}: no zeros, every product matters."""
    return [EXACT_VALUES[rng.integers(0, 4, s)] for s in sizes]


def assert_exact_range(abssum):
    """Every partial sum of an entry, in any order, is a multiple of 1/2 below 2^23 in magnitude: fp32 holds each exactly
    (the issue's 2^24 for integers; one bit less because alpha or beta may be 1/2)."""
    assert abssum.size == 0 or float(abssum.max()) < 2 ** 23, f"exact data leave the exact range: {abssum.max()}"


def check_structure(rowptr, colind, plan, what=""):
    """Row offsets and columns (ascending within each row) equal the reference's, exactly."""
    rowptr, colind = np.asarray(rowptr), np.asarray(colind)
    assert rowptr.shape == plan.rowptr.shape and np.array_equal(rowptr, plan.rowptr), f"{what}: row offsets differ"
    bad = np.flatnonzero(colind[:plan.nnz] != plan.colind)
    if colind.size < plan.nnz or bad.size:
        rows = np.searchsorted(plan.rowptr, bad[:5], side="right") - 1
        raise AssertionError(f"{what}: {bad.size} column indices differ, first in rows {rows.tolist()}")


def check_spg_exact(vt, values, ref, what=""):
    check_exact(vt, torch.as_tensor(np.asarray(values)), ref, what)


def check_spg_random(vt, values, ref, abssum, terms, what=""):
    """Per ENTRY: |error| <= max(util.TOL, (t + 2) / 2 * eps) * sum |terms|, t the number of terms of that entry (t roundings
    of the sum, one of the product, one of the factor; half an eps each)."""
    dt = np.dtype(NUMPY_OF[vt])
    tol = np.maximum(util.TOL[dt], (np.asarray(terms, np.float64) + 2.0) / 2.0 * float(np.finfo(dt).eps))
    err = np.abs(np.asarray(values, np.float64) - ref)
    bound = tol * abssum + float(np.finfo(dt).tiny)
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {bad.sum()} entries out of bound, first at {np.flatnonzero(bad)[:5].tolist()}; " \
                          f"worst ratio {(err / bound).max():.3g}"
