"""Full-output references in float64, written in plain torch so they run on whatever device holds the operands.

The full-size tests compare EVERY output with these, not a sample: a wrong slice or bin boundary that touches a few
hundred rows, two rows' results exchanged, or a lost sign all pass a checksum, linearity and a 6 000-row sample.
Nothing here calls the library: row ids come from repeat_interleave over the row offsets, products are summed in
float64 (index_add_; segment_reduce for SpMM), and SpGEMM's structure comes from an independent expansion of every product to a (row, column)
key.  Work is done in chunks of CHUNK entries (products) so the intermediates stay at a few GB.

fp64 operands are better checked against the host oracle: atomic float64 sums here can carry about k * eps * |row| of
their own error on rows of ~1e5 entries, which is the size of the fp64 bound itself.
"""
import numpy as np
import torch

CHUNK = 1 << 26

TOL = {np.dtype(np.float32): 1e-6, np.dtype(np.float64): 1e-12}  # util.TOL: the parity bound of this build


def _np_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        return np.dtype(str(dtype).replace("torch.", ""))
    return np.dtype(dtype)


def _row_span(rp, e0, e1):
    """(r0, lens): the rows that hold entries [e0, e1) are r0 .. r0 + len(lens) - 1, lens = their entries inside the range
    (rp: int64 row offsets)."""
    ends = torch.tensor([e0, e1 - 1], dtype=torch.int64, device=rp.device)
    r0, r1 = (torch.searchsorted(rp, ends, right=True) - 1).tolist()
    return r0, rp[r0 + 1:r1 + 2].clamp(max=e1) - rp[r0:r1 + 1].clamp(min=e0)


def _rows_of(rp, e0, e1):
    """The row of every entry in [e0, e1)."""
    r0, lens = _row_span(rp, e0, e1)
    return torch.repeat_interleave(torch.arange(r0, r0 + lens.numel(), device=rp.device), lens)


def _entry_chunks(rowptr, chunk, bounds=None):
    """(e0, e1, rows): consecutive ranges of at most `chunk` entries (or between the given `bounds`) and the row of
    every entry in the range."""
    rp = rowptr.long()
    nnz = int(rp[-1])
    if bounds is None:
        bounds = list(range(0, nnz, chunk)) + [nnz]
    for e0, e1 in zip(bounds[:-1], bounds[1:]):
        if e1 > e0:
            yield e0, e1, _rows_of(rp, e0, e1)


def spmv_ref_f64(rowptr, colind, values, x, scale=1.0, chunk=CHUNK):
    """y = scale * A x and absrow = |scale| * sum_p |a_p x_p| per row, both float64."""
    m = rowptr.numel() - 1
    y = torch.zeros(m, dtype=torch.float64, device=values.device)
    absrow = torch.zeros(m, dtype=torch.float64, device=values.device)
    xd = x.double()
    for e0, e1, rows in _entry_chunks(rowptr, chunk):
        prod = values[e0:e1].double() * xd[colind[e0:e1].long()]
        y.index_add_(0, rows, prod)
        absrow.index_add_(0, rows, prod.abs_())
        del prod, rows
    return y.mul_(scale), absrow.mul_(abs(scale))


def spmm_ref_f64(rowptr, colind, values, B, scale=1.0, col_block=16, chunk=CHUNK):
    """C = scale * A B and |scale| * |A| |B| elementwise, float64, over blocks of `col_block` columns of B.  Rows are
    summed with segment_reduce, one sequential sum per (row, column): index_add_ here would put every entry of a hub
    row (1e5 of them in an R-MAT matrix) onto the same 16 addresses at once."""
    rp = rowptr.long()
    m, n, nnz = rp.numel() - 1, B.shape[1], int(rp[-1])
    C = torch.zeros((m, n), dtype=torch.float64, device=values.device)
    Cabs = torch.zeros((m, n), dtype=torch.float64, device=values.device)
    for c0 in range(0, n, col_block):
        c1 = min(n, c0 + col_block)
        for e0 in range(0, nnz, chunk):
            e1 = min(nnz, e0 + chunk)
            r0, lens = _row_span(rp, e0, e1)
            prod = B[colind[e0:e1].long(), c0:c1].double().mul_(values[e0:e1].double()[:, None])
            C[r0:r0 + lens.numel(), c0:c1] += torch.segment_reduce(prod, "sum", lengths=lens, axis=0, unsafe=True,
                                                                   initial=0.0)
            Cabs[r0:r0 + lens.numel(), c0:c1] += torch.segment_reduce(prod.abs_(), "sum", lengths=lens, axis=0,
                                                                      unsafe=True, initial=0.0)
            del prod
    return C.mul_(scale), Cabs.mul_(abs(scale))


def spgemm_ref_f64(A, B, C_rowptr, C_colind, alpha=1.0, D=None, beta=0.0, chunk=CHUNK):
    """Values of C = alpha A B (+ beta D) on C's own structure, float64: returns (c_ref, c_abs) aligned with C_colind.

    A, B, D are (rowptr, colind, values).  Every product a_ik * b_kj and every d_ij is expanded to the key i * n + j and
    located in C's keys with searchsorted.  Asserted on the way, which pins the structure exactly: C's row offsets are a
    valid CSR, its columns strictly ascend within every row, every product (and addend entry) finds its key in C, and
    every entry of C receives at least one of them."""
    dev = C_colind.device
    crp = C_rowptr.long()
    cnnz = int(crp[-1])
    assert int(crp[0]) == 0 and C_colind.numel() >= cnnz, "C row offsets"
    clen = crp[1:] - crp[:-1]
    assert bool((clen >= 0).all()), "C row offsets must not decrease"
    ccol = C_colind[:cnnz].long()
    parts = [B[1][:int(B[0][-1])], ccol] + ([D[1][:int(D[0][-1])]] if D is not None else [])
    n = 1 + max([int(p.max()) for p in parts if p.numel()] + [0])
    assert cnnz == 0 or int(ccol.min()) >= 0, "negative column index in C"
    keys = torch.repeat_interleave(torch.arange(crp.numel() - 1, device=dev), clen).mul_(n).add_(ccol)
    assert bool((keys[1:] > keys[:-1]).all()), "C's columns are not strictly ascending within every row"
    c_ref = torch.zeros(cnnz, dtype=torch.float64, device=dev)
    c_abs = torch.zeros(cnnz, dtype=torch.float64, device=dev)
    hit = torch.zeros(cnnz, dtype=torch.bool, device=dev)

    def scatter(key, val, what):
        loc = torch.searchsorted(keys, key)
        if cnnz:
            found = (loc < cnnz) & (keys[loc.clamp(max=cnnz - 1)] == key)
        else:
            found = torch.zeros_like(key, dtype=torch.bool)
        if not bool(found.all()):
            bad = key[~found][:8].tolist()
            raise AssertionError(f"{what}: {int((~found).sum())} (row, column) pairs missing from C, first "
                                 f"{[(k // n, k % n) for k in bad]}")
        c_ref.index_add_(0, loc, val)
        c_abs.index_add_(0, loc, val.abs())
        hit[loc] = True

    brp, bcol, bval = B[0].long(), B[1], B[2]
    blen = brp[1:] - brp[:-1]
    annz = int(A[0][-1])
    # A entries in ranges whose products number at most `chunk` (one A entry may exceed it on its own)
    cum = torch.cumsum(blen[A[1][:annz].long()], 0)
    marks = torch.arange(chunk, max(int(cum[-1]) if annz else 0, chunk), chunk, device=dev)
    bounds = sorted(set([0, annz] + torch.searchsorted(cum, marks, right=True).tolist()))
    del cum, marks
    for e0, e1, arows in _entry_chunks(A[0], chunk, bounds):
        acol = A[1][e0:e1].long()
        cnt = blen[acol]
        total = int(cnt.sum())
        if total == 0:
            continue
        owner = torch.repeat_interleave(torch.arange(e1 - e0, device=dev), cnt)
        first = torch.cumsum(cnt, 0) - cnt
        bidx = brp[acol][owner] + (torch.arange(total, device=dev) - first[owner])
        key = arows[owner] * n + bcol[bidx].long()
        val = A[2][e0:e1].double()[owner] * bval[bidx].double()
        scatter(key, val.mul_(alpha), "A B")
        del owner, first, bidx, key, val
    if D is not None:  # (beta == 0: D's structure still belongs to C, its values add zeros)
        for e0, e1, drows in _entry_chunks(D[0], chunk):
            scatter(drows * n + D[1][e0:e1].long(), D[2][e0:e1].double() * beta, "D")
    del keys
    if not bool(hit.all()):
        bad = torch.nonzero(~hit).flatten()[:8]
        raise AssertionError(f"{int((~hit).sum())} entries of C receive no product, first positions {bad.tolist()}")
    return c_ref, c_abs


def assert_parity_t(got, ref, absref, dtype, row_len=None, what=""):
    """util.assert_parity evaluated with torch on the tensors' device: norm-wise
    |got - ref| <= max(TOL, row_len / 2 * eps) * absref + tiny, NaN fails.  row_len (per row) broadcasts over
    the trailing dimensions of got."""
    dt = _np_dtype(dtype)
    fi = np.finfo(dt)
    dev = got.device
    ref = torch.as_tensor(ref, device=dev).double()
    absref = torch.as_tensor(absref, device=dev).double()
    tol = torch.full(absref.shape, TOL[dt], dtype=torch.float64, device=dev)
    if row_len is not None:
        rl = torch.as_tensor(np.asarray(row_len) if not torch.is_tensor(row_len) else row_len, device=dev).double()
        rl = rl.reshape((-1,) + (1,) * (absref.dim() - 1))
        tol = torch.maximum(tol, rl * 0.5 * float(fi.eps))
    err = (got.double() - ref).abs_()
    bound = tol.mul_(absref).add_(float(fi.tiny))
    bad = ~(err <= bound)  # NaN (an output the kernel never wrote) must fail, not slip through
    if bool(bad.any()):
        ratio = torch.nan_to_num(err / bound.clamp(min=1e-300), nan=float("inf"))
        idx = torch.nonzero(bad)[:8]
        first = [(tuple(i) if len(i) > 1 else i[0], float(got[tuple(i)]), float(ref[tuple(i)])) for i in idx.tolist()]
        raise AssertionError(f"{what}: {int(bad.sum())} entries exceed the parity bound; worst ratio "
                             f"{float(ratio.max()):.3g}; first (index, got, ref): {first}")
