"""Device side of the SpGEMM / add ladder (tests/ladder.py): one function per operation that runs a matrix triple through the
library -- the symbolic pass, then several numeric passes on the one state with new values and new factors, the result
arrays poisoned before each -- and compares EVERY entry with ladder.SpgemmPlan.  Shared by tests/test_gpu_spgemm_ladders.py
and its child processes (tests/spg_ladder_worker.py)."""
import os

import numpy as np
import torch

import gpu_util as G
import ladder as L
import spblas_reference_amd as sp

PASSES = 5
_PLANS = {}


class Case:
    """A matrix triple with a name: the arrays of a family or of one of the small generators."""

    def __init__(self, name, ar, ac, br, bc, dr, dc, shape):
        self.name, self.ar, self.ac, self.br, self.bc, self.dr, self.dc, self.shape = name, ar, ac, br, bc, dr, dc, shape


def family_case(sub, aclass):
    f = L.spg_family(sub, aclass)
    return Case(f.name, f.ar, f.ac, f.br, f.bc, f.dr, f.dc, (f.m, f.k, f.n))


def family_add_case(sub, aclass):
    """add(): A taken as an m x n matrix and the family's second summand."""
    f = L.spg_family(sub, aclass)
    return Case(f.name + "_add", f.ar, f.ac, None, None, f.add_dr, f.add_dc, (f.m, f.n, f.n))


def plan_of(case, addend):
    key = (case.name, case.shape, addend)
    if key not in _PLANS:
        _PLANS[key] = L.SpgemmPlan(case.ar, case.ac, case.br, case.bc, case.shape, case.dr if addend else None,
                                   case.dc if addend else None)
    return _PLANS[key]


def _values(rng, vt, exact, sizes):
    if exact:
        return L.exact_spg_values(rng, sizes)
    return [L.wide(L.cast(vt, L.random_real(rng, s))) for s in sizes]        # as the value type holds them


def _factor(rng, vt, exact, it):
    if exact:
        return L.EXACT_FACTORS[(it + int(rng.integers(0, 3))) % 3]
    return float(L.wide(L.cast(vt, np.array([rng.uniform(-2, 2)])))[0])


def _check_values(vt, exact, got, plan, av, bv, alpha, dv, beta, what):
    ref, abssum = plan.values(av, bv, alpha, dv, beta)
    if exact:
        L.assert_exact_range(abssum)
        L.check_spg_exact(vt, got, ref, what)
    else:
        L.check_spg_random(vt, got, ref, abssum, plan.terms, what)


def expected_ranked(fills, addend, pred, reuse):
    """fills_by_rank after `fills` numeric passes (spgemm_numeric_typed): the pass that records is the second (the first with
    SPBLAS_GFX950_SPGEMM_REUSE=2, none with =0); never with an addend next to sortable rows; only with rows in bins 1 - 3."""
    small = pred["bin1_rows"] + pred["wave_per_row_rows"] + pred["bin3_rows"]
    return reuse != "0" and fills >= (1 if reuse == "2" else 2) and not (addend and pred["direct_rows"] > 0) and small > 0


def run_product(case, vt, exact, addend, passes=PASSES, seed=7, classify_kw=None, check_info=True):
    """Three-argument (addend=False) or four-argument product.  Returns the number of entries compared."""
    m, k, n = case.shape
    dt = L.TORCH_OF[vt]
    plan = plan_of(case, addend)
    pred = L.predicted_info(case.ar, case.ac, case.br, case.dr if addend else None, **(classify_kw or {}))
    reuse = os.environ.get("SPBLAS_GFX950_SPGEMM_REUSE", "1")[:1]
    what = f"{case.name} {vt} {'EXACT' if exact else 'RANDOM'} {'A*B+D' if addend else 'A*B'}"
    dev = "cuda"
    d_a = sp.csr_view(torch.zeros(case.ac.size, dtype=dt, device=dev), G.dev(case.ar), G.dev(case.ac), (m, k), case.ac.size)
    d_b = sp.csr_view(torch.zeros(case.bc.size, dtype=dt, device=dev), G.dev(case.br), G.dev(case.bc), (k, n), case.bc.size)
    d_d = sp.csr_view(torch.zeros(case.dc.size, dtype=dt, device=dev), G.dev(case.dr), G.dev(case.dc), (m, n),
                      case.dc.size) if addend else None
    d_rp = torch.full((m + 1,), -1, dtype=torch.int32, device=dev)
    d_c = sp.csr_view(None, d_rp, None, (m, n), 0)
    state = sp.spgemm_state_t()
    if addend:
        sp.multiply_compute(state, d_a, d_b, d_c, d_d)
    else:
        sp.multiply_compute(state, d_a, d_b, d_c)
    assert state.result_nnz() == plan.nnz, f"{what}: result_nnz {state.result_nnz()} != {plan.nnz}"
    assert np.array_equal(G.host(d_rp), plan.rowptr), f"{what}: row offsets of the symbolic pass differ"
    info = state.info()
    if check_info:
        for key in ("wave_per_row_rows", "direct_rows", "lanes_per_b_row", "bin1_rows", "bin3_rows", "dense_rows"):
            assert info[key] == pred[key], f"{what}: info[{key}] = {info[key]}, the classification rule gives {pred[key]}"
        assert m - sum(info[x] for x in ("wave_per_row_rows", "bin1_rows", "bin3_rows", "dense_rows")) - pred["empty_rows"] \
            == pred["bin4_rows"], f"{what}: rows of bin 4"
    assert not info["fills_by_rank"]
    nnz = plan.nnz
    vals = torch.empty(nnz, dtype=dt, device=dev)
    cols = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_c.update(vals, d_rp, cols, (m, n), nnz)
    rng = np.random.default_rng(seed)
    compared = 0
    for it in range(passes):
        av, bv, dv = _values(rng, vt, exact, (case.ac.size, case.bc.size, case.dc.size if addend else 0))
        alpha, beta = _factor(rng, vt, exact, it), _factor(rng, vt, exact, it + 1)
        d_a.values().copy_(L.cast(vt, av))
        d_b.values().copy_(L.cast(vt, bv))
        A = sp.scaled(alpha, d_a) if alpha != 1.0 else d_a
        vals.fill_(float("nan"))
        cols.fill_(-7)
        d_rp.fill_(-1)
        fill = sp.multiply_fill if it == 0 else sp.multiply_numeric
        if addend:
            d_d.values().copy_(L.cast(vt, dv))
            fill(state, A, d_b, d_c, sp.scaled(beta, d_d))
        else:
            fill(state, A, d_b, d_c)
        w = f"{what} pass {it + 1}"
        L.check_structure(G.host(d_rp), G.host(cols), plan, w)
        _check_values(vt, exact, G.host(vals), plan, av, bv, alpha, dv if addend else None, beta, w)
        compared += nnz
        if check_info:
            want = expected_ranked(it + 1, addend, pred, reuse)
            assert state.info()["fills_by_rank"] == want, f"{w}: fills_by_rank is {not want}, expected {want}"
    return compared


def run_add(case, vt, exact, passes=PASSES, seed=11):
    """add_inspect + `passes` add_compute on the one state, then the one-shot add() into a pre-sized C; scaled views."""
    m, _, n = case.shape
    dt = L.TORCH_OF[vt]
    plan = plan_of(case, True)
    pred = L.predicted_info(case.ar, case.ac, None, case.dr, identity_b=True)
    what = f"{case.name} {vt} {'EXACT' if exact else 'RANDOM'} add"
    dev = "cuda"
    d_a = sp.csr_view(torch.zeros(case.ac.size, dtype=dt, device=dev), G.dev(case.ar), G.dev(case.ac), (m, n), case.ac.size)
    d_d = sp.csr_view(torch.zeros(case.dc.size, dtype=dt, device=dev), G.dev(case.dr), G.dev(case.dc), (m, n), case.dc.size)
    d_rp = torch.full((m + 1,), -1, dtype=torch.int32, device=dev)
    d_c = sp.csr_view(None, d_rp, None, (m, n), 0)
    info = sp.add_inspect(d_a, d_d, d_c)
    assert info.result_nnz() == plan.nnz, f"{what}: result_nnz {info.result_nnz()} != {plan.nnz}"
    assert np.array_equal(G.host(d_rp), plan.rowptr), f"{what}: row offsets of add_inspect differ"
    got = info.state_.info()
    for key in ("wave_per_row_rows", "direct_rows", "lanes_per_b_row", "bin1_rows", "bin3_rows", "dense_rows"):
        assert got[key] == pred[key], f"{what}: info[{key}] = {got[key]}, the classification rule gives {pred[key]}"
    nnz = plan.nnz
    vals = torch.empty(nnz, dtype=dt, device=dev)
    cols = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_c.update(vals, d_rp, cols, (m, n), nnz)
    rng = np.random.default_rng(seed)
    compared = 0
    for it in range(passes + 1):
        av, dv = _values(rng, vt, exact, (case.ac.size, case.dc.size))
        alpha, beta = _factor(rng, vt, exact, it), _factor(rng, vt, exact, it + 2)
        d_a.values().copy_(L.cast(vt, av))
        d_d.values().copy_(L.cast(vt, dv))
        vals.fill_(float("nan"))
        cols.fill_(-7)
        d_rp.fill_(-1)
        A = sp.scaled(alpha, d_a) if alpha != 1.0 else d_a
        D = sp.scaled(beta, d_d) if beta != 1.0 else d_d
        if it < passes:
            sp.add_compute(info, A, D, d_c)
            w = f"{what} pass {it + 1}"
            want = expected_ranked(it + 1, False, pred, os.environ.get("SPBLAS_GFX950_SPGEMM_REUSE", "1")[:1])
            assert info.state_.info()["fills_by_rank"] == want, f"{w}: fills_by_rank is {not want}, expected {want}"
        else:
            sp.add(A, D, d_c)                                  # one shot into the pre-sized arrays
            w = f"{what} one-shot"
        L.check_structure(G.host(d_rp), G.host(cols), plan, w)
        _check_values(vt, exact, G.host(vals), plan, av, None, alpha, dv, beta, w)
        compared += nnz
    return compared
