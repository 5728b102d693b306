"""CPU tests (-m "not gpu") of tests/fullcheck.py, the float64 references the full-size GPU tests compare every output with.

(1) The helpers agree with the oracle on small cases that have signed data, repeated (row, column) pairs, empty rows and a
hub row, with chunk sizes small enough that rows straddle chunks.  (2) Each corruption a subtly wrong kernel could make
-- rows exchanged, a product dropped, a sign lost, a NaN, an error of twice the bound, a column index off by one, an entry
missing or extra -- fails the check; an error of half the bound passes.  (3) assert_parity_t accepts exactly what
util.assert_parity accepts.
"""
import numpy as np
import pytest
import torch

import fullcheck as F
import util
from oracle import oracle

t = torch.from_numpy


def _csr(m, n, rng, dtype, avg=6, hub=True):
    """Signed values, Poisson row lengths, every 7th row empty, one hub row of 3n entries (so it repeats columns), and a
    repeated (row, column) pair in every 5th row that has two entries or more."""
    lens = rng.poisson(avg, m)
    lens[::7] = 0
    if hub:
        lens[m // 2] = 3 * n
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colind = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    for r in range(0, m, 5):
        if lens[r] >= 2:
            colind[rowptr[r] + 1] = colind[rowptr[r]]
    values = (rng.random(int(rowptr[-1])) - 0.5).astype(dtype)
    return rowptr, colind, values


def _sorted_csr(m, n, rng, dtype, per=4):
    """Distinct columns ascending within each row (the addend of the 4-argument SpGEMM), signed values."""
    rows, cols = [], []
    for r in range(m):
        if r % 6 == 0:
            continue
        c = np.sort(rng.choice(n, size=min(n, per), replace=False))
        rows.append(np.full(len(c), r))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    return rowptr, cols.astype(np.int32), (rng.random(len(cols)) - 0.5).astype(dtype)


# ------------------------------------------------------------------------------------------------ (1) against the oracle
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("chunk", [F.CHUNK, 37])
def test_spmv_ref_matches_the_oracle(dtype, chunk):
    rng = np.random.default_rng(1)
    m, n = 300, 80
    rowptr, colind, values = _csr(m, n, rng, dtype)
    x = (rng.random(n) - 0.5).astype(dtype)
    y, absrow = F.spmv_ref_f64(t(rowptr), t(colind), t(values), t(x), scale=-1.5, chunk=chunk)
    assert y.dtype == absrow.dtype == torch.float64
    y_or = oracle.spmv((m, n), rowptr, colind, values, x, scale_a=-1.5)
    ab_or = 1.5 * oracle.spmv_absrow(rowptr, colind, values, x)
    np.testing.assert_allclose(absrow.numpy(), ab_or, rtol=1e-13, atol=0)
    lens = np.diff(rowptr)
    F.assert_parity_t(t(y_or), y, absrow, dtype, row_len=lens, what="oracle vs spmv_ref_f64")
    assert np.all(y.numpy()[lens == 0] == 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("col_block,chunk", [(16, F.CHUNK), (3, 41)])
def test_spmm_ref_matches_the_oracle(dtype, col_block, chunk):
    rng = np.random.default_rng(2)
    m, k, n = 200, 60, 7
    rowptr, colind, values = _csr(m, k, rng, dtype)
    B = (rng.random((k, n)) - 0.5).astype(dtype)
    C, Cabs = F.spmm_ref_f64(t(rowptr), t(colind), t(values), t(B), scale=2.5, col_block=col_block, chunk=chunk)
    C_or = oracle.spmm((m, k), rowptr, colind, values, B, scale_a=2.5)
    Cabs_or = 2.5 * oracle.spmm((m, k), rowptr, colind, np.abs(values).astype(np.float64), np.abs(B).astype(np.float64))
    np.testing.assert_allclose(Cabs.numpy(), Cabs_or, rtol=1e-13, atol=0)
    F.assert_parity_t(t(C_or), C, Cabs, dtype, row_len=np.diff(rowptr), what="oracle vs spmm_ref_f64")


def _spgemm_case(rng, dtype, m=120, k=90, n=70):
    a = _csr(m, k, rng, dtype, avg=4)
    b = _csr(k, n, rng, dtype, avg=3)
    cap, _ = oracle.spgemm_symbolic((m, k), a[0], a[1], (k, n), b[0], b[1])
    return a, b, cap


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("chunk", [F.CHUNK, 50])
def test_spgemm_ref_matches_the_oracle(dtype, chunk):
    rng = np.random.default_rng(3)
    (ar, ac, av), (br, bc, bv), cap = _spgemm_case(rng, dtype)
    m, k, n = 120, 90, 70
    cr, cc, cv = oracle.spgemm_numeric((m, k), ar, ac, av, (k, n), br, bc, bv, capacity=cap, scale_a=-2.0)
    ref, absref = F.spgemm_ref_f64((t(ar), t(ac), t(av)), (t(br), t(bc), t(bv)), t(cr), t(cc), alpha=-2.0, chunk=chunk)
    assert ref.shape == (cap,)
    _, _, cabs = oracle.spgemm_numeric((m, k), ar, ac, np.abs(av).astype(np.float64), (k, n), br, bc,
                                       np.abs(bv).astype(np.float64), capacity=cap)
    np.testing.assert_allclose(absref.numpy(), 2.0 * cabs, rtol=1e-13, atol=0)
    F.assert_parity_t(t(cv), ref, absref, dtype, what="oracle vs spgemm_ref_f64")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_spgemm_ref_with_an_addend_matches_the_oracle(dtype):
    rng = np.random.default_rng(4)
    m, k, n = 120, 90, 70
    ar, ac, av = _csr(m, k, rng, dtype, avg=4)
    br, bc, bv = _csr(k, n, rng, dtype, avg=3)
    dr, dc, dv = _sorted_csr(m, n, rng, dtype)
    cap, _ = oracle.spgemm_symbolic_d((m, k), ar, ac, (k, n), br, bc, (m, n), dr, dc)
    cr, cc, cv = oracle.spgemm_numeric_d((m, k), ar, ac, av, (k, n), br, bc, bv, (m, n), dr, dc, dv, cap,
                                         alpha=1.5, beta=-0.5)
    ref, absref = F.spgemm_ref_f64((t(ar), t(ac), t(av)), (t(br), t(bc), t(bv)), t(cr), t(cc), alpha=1.5,
                                   D=(t(dr), t(dc), t(dv)), beta=-0.5, chunk=64)
    F.assert_parity_t(t(cv), ref, absref, dtype, what="oracle vs spgemm_ref_f64 with D")


# ------------------------------------------------------------------------------------------------ (2) corruptions
def _spmv_case(dtype=np.float32):
    rng = np.random.default_rng(5)
    m, n = 400, 100
    rowptr, colind, values = _csr(m, n, rng, dtype)
    x = (rng.random(n) - 0.5).astype(dtype)
    y_or = oracle.spmv((m, n), rowptr, colind, values, x)
    y, absrow = F.spmv_ref_f64(t(rowptr), t(colind), t(values), t(x))
    return rowptr, colind, values, x, t(y_or), y, absrow


def _bound(absrow, dtype, lens):
    tol = np.maximum(util.TOL[np.dtype(dtype)], 0.5 * np.asarray(lens, np.float64) * np.finfo(dtype).eps)
    return torch.from_numpy(tol) * absrow + float(np.finfo(dtype).tiny)


def test_the_uncorrupted_output_passes():
    rowptr, _, _, _, got, y, absrow = _spmv_case()
    F.assert_parity_t(got, y, absrow, np.float32, row_len=np.diff(rowptr))


def test_two_rows_swapped_fail():
    rowptr, _, _, _, got, y, absrow = _spmv_case()
    order = torch.argsort(y)
    i, j = int(order[0]), int(order[-1])  # the most negative and the most positive row
    bad = got.clone()
    bad[i], bad[j] = got[j], got[i]
    with pytest.raises(AssertionError, match="2 entries exceed"):
        F.assert_parity_t(bad, y, absrow, np.float32, row_len=np.diff(rowptr))


def test_one_product_dropped_fails():
    rowptr, colind, values, x, got, y, absrow = _spmv_case()
    prod = values.astype(np.float64) * x[colind].astype(np.float64)
    # the smallest product that still stands out of its row's bound: a kernel that skips one entry
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    bound = _bound(absrow, np.float32, np.diff(rowptr)).numpy()[rows]
    p = int(np.flatnonzero(np.abs(prod) > 2 * bound)[np.argmin(np.abs(prod)[np.abs(prod) > 2 * bound])])
    bad = got.clone()
    bad[rows[p]] -= float(prod[p])
    with pytest.raises(AssertionError, match="1 entries exceed"):
        F.assert_parity_t(bad, y, absrow, np.float32, row_len=np.diff(rowptr))


def test_one_sign_flipped_fails():
    rowptr, _, _, _, got, y, absrow = _spmv_case()
    i = int(torch.argmax(y.abs()))
    bad = got.clone()
    bad[i] = -bad[i]
    with pytest.raises(AssertionError, match="1 entries exceed"):
        F.assert_parity_t(bad, y, absrow, np.float32, row_len=np.diff(rowptr))


def test_one_nan_fails_also_in_an_empty_row():
    rowptr, _, _, _, got, y, absrow = _spmv_case()
    for i in (3, 0):  # row 0 is empty: ref 0, bound tiny
        bad = got.clone()
        bad[i] = float("nan")
        with pytest.raises(AssertionError, match="1 entries exceed"):
            F.assert_parity_t(bad, y, absrow, np.float32, row_len=np.diff(rowptr))


@pytest.mark.parametrize("factor,fails", [(2.0, True), (-2.0, True), (0.5, False), (-0.5, False)])
def test_an_error_of_twice_the_bound_fails_and_half_of_it_passes(factor, fails):
    rowptr, _, _, _, _, y, absrow = _spmv_case()
    lens = np.diff(rowptr)
    bound = _bound(absrow, np.float32, lens)
    for i in (1, int(np.argmax(lens)), len(lens) - 1):  # an ordinary row, the hub, the last row
        bad = y.clone()
        bad[i] += factor * bound[i]
        if fails:
            with pytest.raises(AssertionError, match="1 entries exceed"):
                F.assert_parity_t(bad, y, absrow, np.float32, row_len=lens)
        else:
            F.assert_parity_t(bad, y, absrow, np.float32, row_len=lens)


def test_spmm_corruptions_fail():
    rng = np.random.default_rng(6)
    m, k, n = 150, 50, 5
    rowptr, colind, values = _csr(m, k, rng, np.float32)
    B = (rng.random((k, n)) - 0.5).astype(np.float32)
    C, Cabs = F.spmm_ref_f64(t(rowptr), t(colind), t(values), t(B), col_block=2)
    got = t(oracle.spmm((m, k), rowptr, colind, values, B))
    lens = np.diff(rowptr)
    F.assert_parity_t(got, C, Cabs, np.float32, row_len=lens)
    i = int(np.argmax(lens))
    for corrupt in ("swap", "sign", "nan", "column"):
        bad = got.clone()
        if corrupt == "swap":
            bad[[i, i + 1]] = got[[i + 1, i]]
        elif corrupt == "sign":
            bad[i, 3] = -bad[i, 3]
        elif corrupt == "nan":
            bad[i, 4] = float("nan")
        else:  # one output column shifted into the next
            bad[:, 1] = got[:, 2]
        with pytest.raises(AssertionError, match="exceed the parity bound"):
            F.assert_parity_t(bad, C, Cabs, np.float32, row_len=lens, what=corrupt)


def _spgemm_oracle_case():
    rng = np.random.default_rng(7)
    (ar, ac, av), (br, bc, bv), cap = _spgemm_case(rng, np.float32)
    cr, cc, cv = oracle.spgemm_numeric((120, 90), ar, ac, av, (90, 70), br, bc, bv, capacity=cap)
    return (t(ar), t(ac), t(av)), (t(br), t(bc), t(bv)), cr, cc, cv


def test_spgemm_value_corruptions_fail():
    A, B, cr, cc, cv = _spgemm_oracle_case()
    ref, absref = F.spgemm_ref_f64(A, B, t(cr), t(cc))
    F.assert_parity_t(t(cv), ref, absref, np.float32)
    # one product dropped: the entry of C that one product a_ik b_kj lands in, minus that product
    ar, ac, av = (x.numpy() for x in A)
    br, bc, bv = (x.numpy() for x in B)
    r = int(np.argmax(np.diff(ar) * (np.diff(ar) < 20)))  # a row of several entries, not the hub
    p = ar[r]
    q = br[ac[p]]
    while q == br[ac[p] + 1]:  # an entry of A whose row of B is not empty
        p += 1
        q = br[ac[p]]
    pos = cr[r] + int(np.searchsorted(cc[cr[r]:cr[r + 1]], bc[q]))
    for corrupt in ("drop", "sign", "nan", "swap"):
        bad = t(cv.copy())
        if corrupt == "drop":
            bad[pos] -= float(av[p]) * float(bv[q])
            assert abs(float(av[p]) * float(bv[q])) > 2e-6 * float(absref[pos])  # the product stands out of the bound
        elif corrupt == "sign":
            bad[pos] = -bad[pos]
        elif corrupt == "nan":
            bad[pos] = float("nan")
        else:
            j = int(torch.argmax(ref))
            k = int(torch.argmin(ref))
            bad[[j, k]] = t(cv[[k, j]])
        with pytest.raises(AssertionError, match="exceed the parity bound"):
            F.assert_parity_t(bad, ref, absref, np.float32, what=corrupt)


def test_spgemm_structure_corruptions_fail():
    A, B, cr, cc, cv = _spgemm_oracle_case()
    r = int(np.argmax(np.diff(cr) * (np.diff(cr) < 40)))  # a row of several entries
    lo, hi = int(cr[r]), int(cr[r + 1])
    # a column index off by one, at a position where it keeps the row ascending (the product lands nowhere)
    gaps = np.flatnonzero(cc[lo + 1:hi] - cc[lo:hi - 1] > 1)
    assert len(gaps)
    cc1 = cc.copy()
    cc1[lo + gaps[0]] += 1
    with pytest.raises(AssertionError, match="missing from C"):
        F.spgemm_ref_f64(A, B, t(cr), t(cc1))
    # ... and one that collides with its neighbour (not strictly ascending any more)
    adj = np.flatnonzero(cc[lo + 1:hi] - cc[lo:hi - 1] == 1)
    if len(adj):
        cc2 = cc.copy()
        cc2[lo + adj[0]] += 1
        with pytest.raises(AssertionError, match="strictly ascending"):
            F.spgemm_ref_f64(A, B, t(cr), t(cc2))
    # an entry missing: drop position lo + 1 from row r
    cc3 = np.delete(cc, lo + 1)
    cr3 = cr.copy()
    cr3[r + 1:] -= 1
    with pytest.raises(AssertionError, match="missing from C"):
        F.spgemm_ref_f64(A, B, t(cr3), t(cc3))
    # an extra entry: a column no product reaches, inserted in order into row r
    free = np.setdiff1d(np.arange(70), cc[lo:hi])
    extra = int(free[0])
    ins = lo + int(np.searchsorted(cc[lo:hi], extra))
    cc4 = np.insert(cc, ins, extra)
    cr4 = cr.copy()
    cr4[r + 1:] += 1
    with pytest.raises(AssertionError, match="receive no product"):
        F.spgemm_ref_f64(A, B, t(cr4), t(cc4))
    # rows exchanged in the structure: the row offsets say one thing, the columns another
    cr5 = cr.copy()
    cr5[r + 1] += 1
    with pytest.raises(AssertionError):
        F.spgemm_ref_f64(A, B, t(cr5), t(cc))


def test_spgemm_addend_structure_is_part_of_c():
    """With D, an entry only D reaches belongs to C; leaving D's entries out of C is caught."""
    rng = np.random.default_rng(8)
    m, k, n = 60, 40, 50
    ar, ac, av = _csr(m, k, rng, np.float32, avg=2, hub=False)
    br, bc, bv = _csr(k, n, rng, np.float32, avg=2, hub=False)
    dr, dc, dv = _sorted_csr(m, n, rng, np.float32, per=6)
    A, B, D = (t(ar), t(ac), t(av)), (t(br), t(bc), t(bv)), (t(dr), t(dc), t(dv))
    cap, _ = oracle.spgemm_symbolic_d((m, k), ar, ac, (k, n), br, bc, (m, n), dr, dc)
    cr, cc, cv = oracle.spgemm_numeric_d((m, k), ar, ac, av, (k, n), br, bc, bv, (m, n), dr, dc, dv, cap, 2.0, 3.0)
    ref, absref = F.spgemm_ref_f64(A, B, t(cr), t(cc), alpha=2.0, D=D, beta=3.0)
    F.assert_parity_t(t(cv), ref, absref, np.float32)
    # C = A B alone lacks D's own entries
    cap2, _ = oracle.spgemm_symbolic((m, k), ar, ac, (k, n), br, bc)
    cr2, cc2, _ = oracle.spgemm_numeric((m, k), ar, ac, av, (k, n), br, bc, bv, capacity=cap2)
    assert cap2 < cap
    with pytest.raises(AssertionError, match="D: .* missing from C"):
        F.spgemm_ref_f64(A, B, t(cr2), t(cc2), alpha=2.0, D=D, beta=3.0)


# ------------------------------------------------------------------------------------------------ (3) same verdicts
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_assert_parity_t_accepts_exactly_what_assert_parity_accepts(dtype):
    rng = np.random.default_rng(9)
    eps = float(np.finfo(dtype).eps)
    verdicts = []
    for trial in range(400):
        rows, cols = (5, None) if trial % 2 else (4, 3)
        shape = (rows,) if cols is None else (rows, cols)
        ref = rng.standard_normal(shape)
        absref = np.abs(ref) + rng.random(shape)
        absref[0] = 0.0  # an empty row: only tiny is allowed
        lens = rng.integers(0, 3 * int(util.TOL[np.dtype(dtype)] / eps), rows) if trial % 3 else None
        tol = np.full(shape, util.TOL[np.dtype(dtype)])
        if lens is not None:
            tol = np.maximum(tol, 0.5 * lens.astype(np.float64).reshape((-1,) + (1,) * (len(shape) - 1)) * eps)
        bound = tol * absref + float(np.finfo(dtype).tiny)
        # errors at, just above and just below the bound, and far from it; a NaN now and then
        f = rng.choice([0.0, 0.5, -0.5, 0.999], size=shape)
        f.flat[rng.integers(f.size)] = rng.choice([1.0, np.nextafter(1.0, 2.0), 1.0 + 1e-9, 2.0, -1.0, -1.0000001])
        got = (ref + f * bound).astype(dtype if trial % 4 == 0 else np.float64)
        if trial % 17 == 0:
            got.flat[rng.integers(got.size)] = np.nan
        ok_np = ok_t = True
        try:
            util.assert_parity(got, ref, absref, dtype, row_len=lens)
        except AssertionError:
            ok_np = False
        try:
            F.assert_parity_t(t(got), t(ref), t(absref), dtype, row_len=lens)
        except AssertionError:
            ok_t = False
        assert ok_np == ok_t, (trial, got, ref, absref, lens)
        verdicts.append(ok_np)
    assert 0.2 < np.mean(verdicts) < 0.8  # both verdicts were exercised


def test_assert_parity_t_takes_torch_dtypes_and_reports_where():
    ref = torch.tensor([1.0, -2.0, 3.0], dtype=torch.float64)
    got = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float32)
    with pytest.raises(AssertionError, match=r"cfgX: 1 entries exceed .*\(1, 2.0, -2.0\)"):
        F.assert_parity_t(got, ref, ref.abs(), torch.float32, what="cfgX")
