"""-m gpu: what the solver-side inspects share (csrc/csr_inspect.hpp) seen through every inspect that uses it -- the one
lanes-per-row rule at each of its steps, and one table of bad structures / bad perms through every inspect that checks them.
The generators of the bad cases: tests/gs_util.py (proved on the host by tests/test_gs_cpu.py)."""
import numpy as np
import pytest
import torch

import gpu_util as G
import gs_util as GS
import ladder_tt as TT
import spblas_reference_amd as sp

pytestmark = pytest.mark.gpu

M = 100
# every row with 6 / 24 / 96 entries, then one row with one entry more: the means 6, 6.01, 24, 24.01, 96, 96.01 against the strict
# comparisons avg > 6, avg > 24, avg > 96 of lanes_per_row
LANES_AT = {600: 4, 601: 8, 2400: 8, 2401: 16, 9600: 16, 9601: 64}
_SYSTEMS = {}


def step_system(nnz):
    """100 rows of nnz // 100 entries (row 0 one more when nnz is odd), columns r, r + 1, ... mod 100 in ascending order -- every
    row stores its diagonal --, the diagonal 2, the rest +-2^-7; on the device as float32."""
    if nnz not in _SYSTEMS:
        k = nnz // M
        rows = [sorted((r + j) % M for j in range(k + (nnz % M if r == 0 else 0))) for r in range(M)]
        rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        colind = np.asarray([c for r in rows for c in r], np.int32)
        assert colind.size == nnz and all(r in rows[r] and (np.diff(rows[r]) > 0).all() for r in range(M))
        rr = np.repeat(np.arange(M), np.diff(rowptr))
        values = np.where(colind == rr, 2.0, np.where((colind + rr) % 2 == 0, 2.0 ** -7, -2.0 ** -7)).astype(np.float32)
        a = sp.csr_view(G.dev(values), G.dev(rowptr), G.dev(colind), (M, M), nnz)
        _SYSTEMS[nnz] = (a, G.dev((np.arange(M) % 7 - 3).astype(np.float32)))
    return _SYSTEMS[nnz]


@pytest.mark.parametrize("nnz", sorted(LANES_AT))
def test_one_lane_rule_in_every_inspect(gpu, nnz):
    a, b = step_system(nnz)
    want = LANES_AT[nnz]
    assert TT.lanes_of(nnz, M) == want
    x = torch.empty_like(b)
    triangles = [(sp.lower_triangle, sp.explicit_diagonal), (sp.upper_triangle, sp.explicit_diagonal)]
    trsv = [sp.triangular_solve_inspect(a, uplo, diag, b, x) for uplo, diag in triangles]
    got = {"lower": trsv[0].state_.info(), "upper": trsv[1].state_.info(), "ilu0": sp.ilu0_inspect(a).state_.info(),
           "multicolor": sp.multicolor_order(a).info(),
           "gauss_seidel": sp.gauss_seidel_inspect(a, G.dev(np.arange(M + 1, dtype=np.int32))).state_.info()}
    assert {k: v["lanes_per_row"] for k, v in got.items()} == dict.fromkeys(got, want)
    # plan-free and planned sweeps take the same lanes: the same bits
    for info, (uplo, diag) in zip(trsv, triangles):
        free, planned = torch.full_like(b, float("nan")), torch.full_like(b, float("nan"))
        sp.triangular_solve_sweeps(a, uplo, diag, b, free, 1)
        sp.triangular_solve_sweeps(info, a, uplo, diag, b, planned, 1)
        f, p = G.host(free), G.host(planned)
        assert np.isfinite(f).all() and (f.view(np.uint32) == p.view(np.uint32)).all()


# ---- one table of bad structures, every inspect that checks structure
def _small():
    return GS.small_system((10, 10, 10, 10), k=2, seed=5)


def _view(rowptr, colind):
    return sp.csr_view(G.dev(np.ones(colind.size, np.float32)), G.dev(rowptr.astype(np.int32)), G.dev(colind.astype(np.int32)),
                       (rowptr.size - 1,) * 2, int(colind.size))


class PoisonedB:
    """b of permute_inspect: arrays of the right sizes filled with values no inspect writes."""

    def __init__(self, m, nnz):
        self.arrays = (torch.full((nnz,), float("nan"), dtype=torch.float32, device="cuda"),
                       torch.full((m + 1,), -7, dtype=torch.int32, device="cuda"),
                       torch.full((nnz,), -7, dtype=torch.int32, device="cuda"))
        self.view = sp.csr_view(*self.arrays, (m, m), nnz)

    def untouched(self):
        v, rp, ci = (G.host(t) for t in self.arrays)
        return np.isnan(v).all() and (rp == -7).all() and (ci == -7).all()


def _inspects(y):
    """name -> the inspect of a view over B's sorted structure (ilu0 wants ascending columns), and the poisoned b of permute."""
    cp, perm = G.dev(y.color_ptr), G.dev(y.perm)
    pb = PoisonedB(y.m, y.nnz)
    return pb, {"multicolor_order": sp.multicolor_order,
                "permute_inspect": lambda a: sp.permute_inspect(a, perm, pb.view),
                "gauss_seidel_inspect": lambda a: sp.gauss_seidel_inspect(a, cp),
                "ilu0_inspect": sp.ilu0_inspect}


def test_the_good_structure_passes_every_inspect(gpu):
    y = _small()
    assert y.m == 40
    pb, inspects = _inspects(y)
    for name, inspect in inspects.items():
        inspect(_view(y.b_rowptr, y.b_colind))
    assert not pb.untouched()


@pytest.mark.parametrize("name", ["multicolor_order", "permute_inspect", "gauss_seidel_inspect", "ilu0_inspect"])
def test_bad_structures_are_refused_by_every_inspect(gpu, name):
    y = _small()
    pb, inspects = _inspects(y)
    cases = GS.bad_structures(y.b_rowptr, y.b_colind)
    assert len(cases) == 4
    for rp, ci in cases:
        with pytest.raises(ValueError):
            inspects[name](_view(rp, ci))
    assert pb.untouched(), "a refused permute_inspect wrote b"


def test_bad_perms_are_refused_by_both_inspects_that_take_one(gpu):
    y = _small()
    a, cp = _view(y.rowptr, y.colind), G.dev(y.color_ptr)
    pb = PoisonedB(y.m, y.nnz)
    sp.gauss_seidel_inspect(a, cp, G.dev(y.perm))           # the good perm passes
    cases = GS.bad_perms(y.perm)
    assert len(cases) == 3
    for p in cases:
        with pytest.raises(ValueError):
            sp.permute_inspect(a, G.dev(p), pb.view)
        with pytest.raises(ValueError):
            sp.gauss_seidel_inspect(a, cp, G.dev(p))
    assert pb.untouched(), "a refused permute_inspect wrote b"
