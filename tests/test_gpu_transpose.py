"""-m gpu: device transpose and the inspected CSC-operand SpMV.
transpose: cases of /root/reference/test/gtest/transpose_test.cpp (util::dims), arrays compared
EXACTLY with the oracle's restatement of algorithms/transpose_impl.hpp:14-53 (stable counting sort:
it is pure data movement, so values are bit-identical too, including duplicate (i,j) entries)."""
import numpy as np
import pytest
import torch

import gpu_util as G
import spblas_reference_amd as sp
import util
from oracle import oracle
from spblas_reference_amd import _capi, generate

pytestmark = pytest.mark.gpu


def device_transpose(values, rowptr, colind, shape, nnz):
    a = G.csr_on_device(values, rowptr, colind, shape, nnz)
    b = sp.csr_view(torch.full((nnz,), float("nan"), dtype=a.values().dtype, device="cuda"),
                    torch.full((shape[1] + 1,), -1, dtype=torch.int32, device="cuda"),
                    torch.full((nnz,), -1, dtype=torch.int32, device="cuda"), (shape[1], shape[0]), nnz)
    info = sp.transpose_inspect(a, b)
    sp.transpose(info, a, b)
    return G.host(b.rowptr()), G.host(b.colind()), G.host(b.values())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dim", util.dims + [(1, 7, 5), (300, 1, 120)])
def test_transpose_matches_reference_exactly(gpu, dim, dtype):
    m, k, nnz = dim
    values, rowptr, colind, shape, nnz = generate.generate_csr(m, k, nnz, dtype=dtype)
    got = device_transpose(values, rowptr, colind, shape, nnz)
    ref = oracle.transpose(shape, rowptr, colind, values)
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)


def test_transpose_duplicates_empty_and_errors(gpu):
    # duplicate (i,j) entries and empty rows/columns: stable order keeps the duplicates' values in place
    rowptr = np.array([0, 3, 3, 6, 7], np.int32)
    colind = np.array([4, 1, 4, 0, 4, 0, 2], np.int32)
    values = np.arange(1, 8, dtype=np.float32)
    got = device_transpose(values, rowptr, colind, (4, 6), 7)
    ref = oracle.transpose((4, 6), rowptr, colind, values)
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    a = G.csr_on_device(values, rowptr, colind, (4, 6), 7)
    with pytest.raises(ValueError):  # transpose_impl.hpp:17-21
        sp.transpose(a, sp.csr_view(torch.zeros(7, device="cuda"), torch.zeros(6, dtype=torch.int32, device="cuda"),
                                    torch.zeros(7, dtype=torch.int32, device="cuda"), (5, 4), 7))
    with pytest.raises(RuntimeError, match="ran out of memory"):  # :22-25
        sp.transpose(a, sp.csr_view(torch.zeros(6, device="cuda"), torch.zeros(7, dtype=torch.int32, device="cuda"),
                                    torch.zeros(6, dtype=torch.int32, device="cuda"), (6, 4), 6))


def _structured(m, n, row_len, cols_of, rng, dtype=np.float32):
    rowptr = np.zeros(m + 1, np.int64)
    rowptr[1:] = np.cumsum(row_len)
    colind = np.concatenate([cols_of(r, int(l)) for r, l in enumerate(row_len)] or [np.zeros(0)]).astype(np.int32)
    return rng.random(len(colind)).astype(dtype), rowptr.astype(np.int32), colind, (m, n), len(colind)


@pytest.mark.parametrize("case", ["one_pass", "two_passes", "four_passes_long_gaps", "mostly_empty_rows",
                                  "one_hot_column", "partial_last_tile_f64"])
def test_transpose_radix_passes_corner_cases(gpu, case):
    """The hand-written radix passes of csrc/transpose.hip against the oracle, bit for bit: 1 / 2 / 4 passes (n <= 256,
    <= 65 536, > 16 M columns), column gaps of every class of the row-offset pass (lane, wave, whole-grid list), tiles
    whose rows are almost all empty (thousands of row starts on one entry), one column that takes everything (a single
    bucket per pass), several tiles with a partial last one, repeated columns inside rows (stability)."""
    rng = np.random.default_rng(17)
    dtype = np.float32
    if case == "one_pass":
        m, n = 3000, 200
        lens = rng.integers(0, 12, m)
        cols = lambda r, l: rng.integers(0, n, l)                      # repeated columns inside a row
    elif case == "two_passes":
        m, n = 2500, 40_000
        lens = rng.integers(0, 15, m)
        cols = lambda r, l: rng.integers(0, n, l)
    elif case == "four_passes_long_gaps":
        m, n = 4000, 20_000_000
        lens = rng.integers(0, 8, m)
        pool = np.concatenate([rng.integers(0, 50, 40), rng.integers(5_000, 9_000, 40),
                               rng.integers(17_000_000, 17_000_300, 60), [n - 1]])
        cols = lambda r, l: rng.choice(pool, l)
    elif case == "mostly_empty_rows":
        m, n = 200_000, 5000
        lens = np.zeros(m, np.int64)
        busy = rng.choice(m, 900, replace=False)
        lens[busy] = rng.integers(1, 30, len(busy))
        lens[:5000] = 0
        lens[-7000:] = 0
        cols = lambda r, l: rng.integers(0, n, l)
    elif case == "one_hot_column":
        m, n = 9000, 70_000
        lens = np.full(m, 2)
        cols = lambda r, l: np.array([4321, 4321 if r % 3 else 69_999])
    else:
        m, n, dtype = 1300, 3000, np.float64
        lens = rng.integers(5, 12, m)                                   # ~ 11 000 entries: three tiles of 4096
        cols = lambda r, l: rng.integers(0, n, l)
    values, rowptr, colind, shape, nnz = _structured(m, n, lens, cols, rng, dtype)
    got = device_transpose(values, rowptr, colind, shape, nnz)
    ref = oracle.transpose(shape, rowptr, colind, values)
    for g, r, what in zip(got, ref, ("rowptr", "colind", "values")):
        assert np.array_equal(g, r), f"{case}: {what} differs"


def test_transpose_large_is_an_involution(gpu):
    m, n = 300_000, 200_000
    values, rowptr, colind, shape, nnz = generate.uniform_csr_device(m, n, 12, seed=4)
    a = sp.csr_view(values, rowptr, colind, shape, nnz)
    mk = lambda rows, cols: sp.csr_view(torch.empty(nnz, device="cuda"), torch.empty(rows + 1, dtype=torch.int32, device="cuda"),
                                        torch.empty(nnz, dtype=torch.int32, device="cuda"), (rows, cols), nnz)
    b, c = mk(n, m), mk(m, n)
    sp.transpose(a, b)
    sp.transpose(b, c)
    # (A^T)^T has A's rows with columns sorted ascending (stable), same multiset of entries
    assert torch.equal(c.rowptr(), rowptr)
    key_a = torch.sort(colind.long() + torch.repeat_interleave(torch.arange(m, device="cuda"), 12) * n).values
    key_c = c.colind().long() + torch.repeat_interleave(torch.arange(m, device="cuda"), 12) * n
    assert torch.equal(key_a, key_c)
    x = torch.rand(n, device="cuda")
    y1, y2 = torch.empty(m, device="cuda"), torch.empty(m, device="cuda")
    sp.multiply(a, x, y1)
    sp.multiply(c, x, y2)
    assert bool(((y1 - y2).abs() <= 2e-6 * y1.abs() + 1e-30).all())


def test_transpose_at_bench_size_is_bit_exact(gpu):
    """B = A^T at the size bench.py --full times: 10M x 10M, 10 entries per row (generate.uniform_csr_device, seed 0).
    Every row offset, column and value bit EXACT against oracle.transpose (the reference's stable counting sort)."""
    m = 10_000_000
    av, ar, ac, ash, annz = generate.uniform_csr_device(m, m, 10, seed=0)
    a = sp.csr_view(av, ar, ac, ash, annz)
    t_rp = torch.full((m + 1,), -1, dtype=torch.int32, device="cuda")
    t_ci = torch.full((annz,), -1, dtype=torch.int32, device="cuda")
    t_v = torch.full((annz,), float("nan"), device="cuda")
    sp.transpose(a, sp.csr_view(t_v, t_rp, t_ci, (m, m), annz))
    r_rp, r_ci, r_v = oracle.transpose((m, m), ar.cpu().numpy(), ac.cpu().numpy(), av.cpu().numpy())
    assert np.array_equal(G.host(t_rp), r_rp), "transpose at bench size: row offsets"
    assert np.array_equal(G.host(t_ci), r_ci), "transpose at bench size: columns"
    assert np.array_equal(G.host(t_v).view(np.uint32), r_v.view(np.uint32)), "transpose at bench size: value bits"


@pytest.mark.parametrize("alg", [_capi.SPMV_AUTO, _capi.SPMV_SLICED])
def test_inspected_csc_operand_uses_regular_kernels(gpu, alg):
    # y = A x with A given as csc_view (test/gtest/spmv_test.cpp:110-208), inspect + execute
    values, rowptr, colind, shape, nnz = generate.generate_csr(700, 900, 15000, seed=12)
    a_t = G.csr_on_device(values, rowptr, colind, shape, nnz)   # stored arrays: CSR of a 700x900 matrix
    a_csc = sp.transposed(a_t)                                   # logical 900x700 operand in CSC
    x_h = np.random.default_rng(1).random(700).astype(np.float32)
    y = torch.full((900,), float("nan"), device="cuda")
    info = sp.multiply_inspect(a_csc, G.dev(x_h), y, alg=alg)
    assert info.state_.info()["alg"] in (_capi.SPMV_ROWBLOCK, _capi.SPMV_SLICED, _capi.SPMV_VECTOR)
    sp.multiply(info, sp.scaled(3.0, a_csc), G.dev(x_h), y)
    y_ref = oracle.spmv_csc((900, 700), rowptr, colind, values, x_h, scale_a=3.0)
    tr, tc, tv = oracle.transpose(shape, rowptr, colind, values)
    absrow = 3.0 * oracle.spmv_absrow(tr, tc, tv, x_h)
    util.assert_parity(G.host(y), y_ref, absrow, np.float32, row_len=np.diff(tr), what="inspected csc spmv")
    # without the info the atomic op=T path gives the same answer
    y2 = torch.zeros(900, device="cuda")
    sp.multiply(sp.scaled(3.0, a_csc), G.dev(x_h), y2)
    util.assert_parity(G.host(y2), y_ref, absrow, np.float32, row_len=np.diff(tr), what="atomic csc spmv")


@pytest.mark.parametrize("hub", [False, True])
def test_inspected_csc_operand_releases_its_row_major_arrays(gpu, hub):
    """Round 6 (review item 4: the inspected transposed operand held 2.43 x the matrix -- the materialised row-major copy next
    to the plan).  When the plan is self-contained (SLICED tiles with their own values, no hub rows: a uniform matrix large
    enough for the tiles) the host layer releases the materialised arrays after spblas_gfx950_spmv_plan_detach and the
    multiplies pass NO matrix arrays; the state then holds the plan alone (<= 1.5 x the matrix).  A matrix with a hub row (its
    entries are multiplied from the arrays at execute time) keeps them.  Either way: results against the oracle, a change of
    the values in place is noticed (the detached form materialises and plans again), SpMM with the SpMV-inspected info
    still works."""
    rng = np.random.default_rng(77)
    k, n_cols, per = 1_000_000, 1_000_000, 10        # stored CSR: k x n_cols; the operand is its transpose, n_cols x k
    lens = np.full(k, per)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(rowptr[-1])
    colind = rng.integers(0, n_cols, nnz).astype(np.int32)
    if hub:
        colind[rng.random(nnz) < 0.3] = 4242         # a hot COLUMN of the stored matrix = a hub ROW of the operand
    values = (rng.random(nnz) - 0.5).astype(np.float32)
    a_csc = sp.transposed(G.csr_on_device(values, rowptr, colind, (k, n_cols), nnz))   # n_cols x k
    x_h = (rng.random(k) - 0.5).astype(np.float32)
    xd = G.dev(x_h)
    y = torch.full((n_cols,), float("nan"), device="cuda")
    info = sp.multiply_inspect(sp.matrix_opt(a_csc), xd, y)
    st = info.state_
    matrix_bytes = nnz * 8 + (k + 1) * 4
    held = st.held_bytes() + st.info()["device_bytes"]
    if hub:
        # (whether this plan is self-contained depends on how the long row is handled -- cut into pieces inside the tiles, or
        # kept out of them as a hub row multiplied from the arrays: the library decides, the results below must hold)
        assert st.detached == (st.held_bytes() == 0)
    else:
        assert st.info()["alg"] == _capi.SPMV_SLICED and st.detached and st.held_bytes() == 0
        # (the plan alone: 1.61 x the matrix at this size, 1.43 x at cfg2's -- bench.py's f_csc_spmv record; with the
        # materialised arrays it was one whole matrix more)
        assert held <= 1.7 * matrix_bytes, (held, matrix_bytes)

    def check(vals, scale, what):
        y_ref = oracle.spmv_csc((n_cols, k), rowptr, colind, vals, x_h, scale_a=scale)
        y_abs = abs(scale) * oracle.spmv_csc((n_cols, k), rowptr, colind, np.abs(vals), np.abs(x_h))
        cnt = np.bincount(colind, minlength=n_cols)
        util.assert_parity(G.host(y), y_ref, y_abs, np.float32, row_len=cnt, what=what)

    sp.multiply(info, sp.scaled(-2.0, a_csc), xd, y)
    check(values, -2.0, f"inspected csc operand, hub={hub}")
    a_csc.values().mul_(0.5).add_(0.125)            # in place (torch bumps the version counter: the layer notices)
    v2 = (values * np.float32(0.5) + np.float32(0.125)).astype(np.float32)
    y.fill_(float("nan"))
    sp.multiply(info, a_csc, xd, y)
    check(v2, 1.0, f"inspected csc operand after an in-place change, hub={hub}")
    assert info.state_.detached == (info.state_.held_bytes() == 0)
    # SpMM with the info of the SpMV inspect
    B = (rng.random((k, 8)) - 0.5).astype(np.float32)
    C = torch.full((n_cols, 8), float("nan"), device="cuda")
    sp.multiply(info, a_csc, G.dev(B), C)
    rows = rng.integers(0, n_cols, 200)
    import scipy.sparse as sps
    At = sps.csr_matrix((v2.astype(np.float64), colind, rowptr), shape=(k, n_cols)).T.tocsr()
    ref = (At[rows] @ B.astype(np.float64))
    ab = (abs(At[rows]) @ np.abs(B).astype(np.float64))
    got = G.host(C)[rows]
    assert (np.abs(got - ref) <= 1e-5 * ab + 1e-30).all()


@pytest.mark.parametrize("inspect", [False, True])
def test_spmm_with_csc_operand(gpu, inspect):
    # CscView.SpMM (test/gtest/spmm_test.cpp:181): C = A B with A held by columns
    values, rowptr, colind, shape, nnz = generate.generate_csr(300, 200, 5000, seed=5)  # CSR of A^T (300x200)
    a_csc = sp.transposed(G.csr_on_device(values, rowptr, colind, shape, nnz))          # A is 200x300
    B_h = generate.generate_dense(300, 24)
    C = torch.full((200, 24), float("nan"), device="cuda")
    if inspect:
        info = sp.multiply_inspect(a_csc, G.dev(B_h), C)
        sp.multiply(info, sp.scaled(0.5, a_csc), G.dev(B_h), C)
    else:
        sp.multiply(sp.scaled(0.5, a_csc), G.dev(B_h), C)
    tr, tc, tv = oracle.transpose(shape, rowptr, colind, values)  # row-major A
    C_ref = oracle.spmm((200, 300), tr, tc, tv, B_h, scale_a=0.5)
    import scipy.sparse as sps
    ab = 0.5 * (sps.csr_matrix((np.abs(tv).astype(np.float64), tc, tr), shape=(200, 300)) @ np.abs(B_h).astype(np.float64))
    util.assert_parity(G.host(C), C_ref, ab, np.float32, row_len=np.diff(tr), what="csc spmm")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scale_in_place_matrix_and_vector(gpu, dtype):
    """scale(alpha, t) (algorithms/scale_impl.hpp:13-31): values[i] *= alpha, bit-exact (one IEEE multiply
    per element); odd lengths and unaligned starts exercise the scalar head and tail of the kernel."""
    rng = np.random.default_rng(5)
    for n, off in [(1, 0), (3, 1), (1000, 0), (4099, 3), (1 << 20, 1)]:
        v = rng.standard_normal(n + off).astype(dtype)
        d = G.dev(v)
        view = d[off:]
        sp.scale(-1.75, view)
        exp = v.copy()
        exp[off:] *= dtype(-1.75)
        assert np.array_equal(G.host(d), exp)
    a_h = generate.generate_csr(300, 200, 5000, dtype=dtype)[:4]
    d_a = G.csr_on_device(*a_h, len(a_h[0]))
    sp.scale(3.0, d_a)
    assert np.array_equal(G.host(d_a.values()), a_h[0] * dtype(3.0))
    x = G.dev((rng.random(200) + 0.5).astype(dtype))  # sign-definite: the reference's comparator applies
    y = torch.empty(300, dtype=x.dtype, device="cuda")
    sp.multiply(d_a, x, y)
    ref = oracle.spmv((300, 200), a_h[1], a_h[2], a_h[0] * dtype(3.0), G.host(x))
    util.expect_eq_ref(ref, G.host(y))


def test_64_bit_offsets_in_transpose_and_inspected_csc(gpu):
    """csr_view / csc_view are templated on the offset type (views/csr_view.hpp): transpose() and multiply_inspect on a
    csc_view take 64-bit offset arrays too (narrowed once on the way into the 32-bit device transpose, widened on the
    way out) and give what the 32-bit call gives."""
    values, rowptr, colind, shape, nnz = generate.generate_csr(700, 900, 15000, seed=13)
    ref = oracle.transpose(shape, rowptr, colind, values)
    a = G.csr_on_device(values, rowptr, colind, shape, nnz, offset64=True)
    assert a.rowptr().dtype == torch.int64
    b = sp.csr_view(torch.full((nnz,), float("nan"), device="cuda"),
                    torch.full((shape[1] + 1,), -1, dtype=torch.int64, device="cuda"),
                    torch.full((nnz,), -1, dtype=torch.int32, device="cuda"), (shape[1], shape[0]), nnz)
    sp.transpose(a, b)
    assert b.rowptr().dtype == torch.int64
    for g, r in zip((G.host(b.rowptr()), G.host(b.colind()), G.host(b.values())), ref):
        assert np.array_equal(g, r)
    # the same arrays as a CSC operand with inspect: SpMV and SpMM
    a_csc = sp.transposed(a)  # logical 900 x 700
    x_h = np.random.default_rng(2).random(700).astype(np.float32)
    y = torch.full((900,), float("nan"), device="cuda")
    info = sp.multiply_inspect(a_csc, G.dev(x_h), y)
    sp.multiply(info, a_csc, G.dev(x_h), y)
    tr, tc, tv = ref
    util.assert_parity(G.host(y), oracle.spmv((900, 700), tr, tc, tv, x_h), oracle.spmv_absrow(tr, tc, tv, x_h),
                       np.float32, row_len=np.diff(tr), what="inspected csc spmv, 64-bit offsets")
    B_h = generate.generate_dense(700, 8)
    C = torch.full((900, 8), float("nan"), device="cuda")
    infoC = sp.multiply_inspect(a_csc, G.dev(B_h), C)
    sp.multiply(infoC, a_csc, G.dev(B_h), C)
    np.testing.assert_allclose(G.host(C), oracle.spmm((900, 700), tr, tc, tv, B_h), rtol=2e-5, atol=1e-6)
