"""Device side of the ladders of tests/ladder_tt.py: one function per operation that runs a case through the library with
poisoned, over-long outputs and compares every element with the reference.  Shared by tests/test_gpu_tt_ladders.py and its
child process (tests/tt_ladder_worker.py)."""
import os

import numpy as np
import torch

import gpu_util as G
import ladder_tt as T
import spblas_reference_amd as sp

TORCH_OF = {"f32": torch.float32, "f64": torch.float64}
NUMPY_OF = {"f32": np.float32, "f64": np.float64}
INT_OF = {4: torch.int32, 8: torch.int64}
SURPLUS = 3


def _window(host, shift, surplus, fill, dtype):
    """(store, view): a device store of shift + len(host) + surplus elements filled with `fill`; the view starts `shift`
    elements in (its base pointer is off by that much) and runs to the store's end; host is copied to its head if given."""
    n = len(host) if not isinstance(host, int) else host
    store = torch.full((shift + n + surplus,), fill, dtype=dtype, device="cuda")
    view = store[shift:]
    if not isinstance(host, int) and n:
        view[:n].copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return store, view


def _same_bits(t, ref):
    return torch.equal(t.contiguous().view(INT_OF[t.element_size()]), ref.contiguous().view(INT_OF[ref.element_size()]))


def run_transpose(case, vt, off64=False, shifts=(0, 0, 0, 0, 0), ref=None):
    """B = A^T of one case: inputs and outputs shifted by `shifts` elements (colind, values, t_rowptr, t_colind, t_values),
    outputs prefilled with -1 / NaN and SURPLUS elements longer than needed.  Row offsets, columns and value bits must equal
    oracle.transpose's, and every element of the stores outside the result must keep its prefill.  Returns the reference."""
    dt, nd = TORCH_OF[vt], NUMPY_OF[vt]
    ot = torch.int64 if off64 else torch.int32
    m, n, nnz = case.m, case.n, case.nnz
    _, ci = _window(case.colind, shifts[0], 0, 0, torch.int32)
    _, va = _window(case.values(nd), shifts[1], 0, 0.0, dt)
    rp = torch.from_numpy(case.rowptr.astype(np.int64 if off64 else np.int32)).cuda()
    a = sp.csr_view(va, rp, ci, (m, n), nnz)
    rp_store, t_rp = _window(n + 1, shifts[2], SURPLUS, -1, ot)
    ci_store, t_ci = _window(nnz, shifts[3], SURPLUS, -1, torch.int32)
    va_store, t_va = _window(nnz, shifts[4], SURPLUS, float("nan"), dt)
    b = sp.csr_view(t_va, t_rp, t_ci, (n, m), nnz)
    sp.transpose(sp.transpose_inspect(a, b), a, b)
    torch.cuda.synchronize()
    if ref is None:
        ref = T.transpose_reference(case, nd)
    what = f"{case.name} {vt} offsets{'64' if off64 else '32'} shifts {shifts}"
    r_rp, r_ci, r_va = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in ref)
    ok = torch.equal(t_rp[:n + 1], r_rp.to(ot)) and torch.equal(t_ci[:nnz], r_ci) and _same_bits(t_va[:nnz], r_va)
    if not ok:
        got = (t_rp[:n + 1].to(torch.int32).cpu().numpy(), t_ci[:nnz].cpu().numpy(), t_va[:nnz].cpu().numpy())
        raise AssertionError(f"{what}: {T.transpose_violations(case, got, ref)}")
    for store, lo, hi, fill in ((rp_store, shifts[2], shifts[2] + n + 1, -1), (ci_store, shifts[3], shifts[3] + nnz, -1),
                                (va_store, shifts[4], shifts[4] + nnz, float("nan"))):
        want = torch.full_like(store, fill)
        assert _same_bits(store[:lo], want[:lo]), f"{what}: elements in front of an output array were written"
        assert _same_bits(store[hi:], want[hi:]) and store[hi:].numel() == SURPLUS, \
            f"{what}: the surplus behind an output array was written"
    return ref


def run_scale(vt, n, off):
    """scale(-1.75, view of n elements that starts `off` elements into its base): the WHOLE base is compared."""
    base, want = T.scale_data(n, off, NUMPY_OF[vt])
    d = G.dev(base)
    sp.scale(-1.75, d[off:off + n])
    torch.cuda.synchronize()
    if not torch.equal(d, G.dev(want)):
        got = d.cpu().numpy()
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"scale {vt} n {n} offset {off}: {bad.size} elements differ, first at {bad[:5].tolist()} "
                             f"(view [{off}, {off + n})): {got[bad[:5]].tolist()} != {want[bad[:5]].tolist()}")


# ------------------------------------------------------------------------------------------------------ triangular solve
def hsa_tool_loaded():
    """(under an HSA tool such as rocprofv3 the default falls back to one launch per level, sptrsv.hip)"""
    return bool(os.environ.get("ROCP_TOOL_LIBRARIES") or os.environ.get("HSA_TOOLS_LIB"))


MODES = {"default": {}, "kahn": {"SPBLAS_GFX950_TRSV_KAHN": "1"}, "coop0": {"SPBLAS_GFX950_TRSV_COOP": "0"},
         "grid3": {"SPBLAS_GFX950_TRSV_COOP_GRID": "3"}, "narrow100000": {"SPBLAS_GFX950_TRSV_NARROW": "100000"}}


def tags(upper, unit):
    return (sp.upper_triangle if upper else sp.lower_triangle, sp.implicit_unit_diagonal if unit else sp.explicit_diagonal)


def inspect(sysm, vt, mode, monkeypatch):
    """(a, A, info): the system on the device with its EXACT values, A = scaled(alpha, a), and its plan made under `mode`;
    what the plan reports must equal what ladder_tt.predicted_info restates."""
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    a = G.csr_on_device(sysm.exact_values.astype(NUMPY_OF[vt]), sysm.rowptr, sysm.colind, (sysm.m, sysm.m), sysm.nnz)
    A = sp.scaled(sysm.alpha, a) if sysm.alpha != 1.0 else a
    uplo, diag = tags(sysm.upper, sysm.unit)
    dt = TORCH_OF[vt]
    info = sp.triangular_solve_inspect(A, uplo, diag, torch.zeros(sysm.m, dtype=dt, device="cuda"),
                                       torch.zeros(sysm.m, dtype=dt, device="cuda"))
    want = T.predicted_info(sysm.rowptr, sysm.colind, sysm.m, sysm.upper,
                            narrow=100000 if mode == "narrow100000" else None,
                            coop=mode != "coop0" and not hsa_tool_loaded())
    got = info.state_.info()
    assert got == want, f"{mode} {vt}: the plan reports {got}, the levels restated on the host give {want}"
    assert want["lanes_per_row"] == sysm.lanes and want["levels"] == len(sysm.widths) and \
        want["max_level_width"] == max(sysm.widths)
    return a, A, info


def solve_exact(sysm, vt, A, info, block=None):
    """x = inv(T) b with x prefilled with NaN; x must EQUAL x_true.  block = (layout of B, layout of X): the same system with
    the three columns of ladder_tt.block_rhs."""
    uplo, diag = tags(sysm.upper, sysm.unit)
    dt = TORCH_OF[vt]
    if block is None:
        b = G.dev(sysm.b.astype(NUMPY_OF[vt]))
        x = torch.full((sysm.m,), float("nan"), dtype=dt, device="cuda")
    else:
        bh = T.block_rhs(sysm).astype(NUMPY_OF[vt])
        b = G.dev(bh) if block[0] == "R" else G.dev(bh).t().contiguous().t()
        x = torch.full(bh.shape if block[1] == "R" else bh.shape[::-1], float("nan"), dtype=dt, device="cuda")
        x = x if block[1] == "R" else x.t()
    sp.triangular_solve(info, A, uplo, diag, b, x)
    info.state_.check_status()
    bad = T.exact_violations(G.host(x), sysm)
    assert not bad, f"{vt} {'vector' if block is None else block}: {bad}"
    return x
