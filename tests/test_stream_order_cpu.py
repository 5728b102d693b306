"""Host-side proof of tests/stream_util.py (no GPU): every exported name that launches device work has a stream-order case or a
reasoned exemption, and every case's generators hold what the device tests rely on -- expected(real) passes the case's own
comparison, expected(decoy) fails it, and the two differ in every output element."""
import ast
import os

import numpy as np
import pytest

import stream_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exported_names():
    """Every name spblas-reference_amd/__init__.py imports into the package, read from its source."""
    with open(os.path.join(ROOT, "spblas-reference_amd", "__init__.py")) as f:
        tree = ast.parse(f.read())
    names = []
    for node in tree.body:
        if isinstance(node, ast.ImportFrom):
            names += [a.asname or a.name for a in node.names]
    assert len(names) > 40, "the export list was not found: update exported_names()"
    return names


def test_every_export_has_a_case_or_an_exemption():
    """A new op cannot be exported without a stream-order case (or a line that says why it needs none)."""
    covered = set()
    for c in S.CASES:
        covered |= set(c.covers) | set(c.uses)
    names = set(exported_names())
    missing = sorted(names - covered - set(S.EXEMPT))
    assert missing == [], f"exported without a case in stream_util.CASES or an entry in stream_util.EXEMPT: {missing}"
    assert sorted(covered - names) == [], "a case names something the package does not export"
    assert sorted(set(S.EXEMPT) - names) == [], "an exemption names something the package does not export"
    assert sorted(set(S.EXEMPT) & covered) == [], "exempted and covered at once"
    assert all(isinstance(why, str) and why for why in S.EXEMPT.values())


def test_the_table_is_well_formed():
    assert len({c.name for c in S.CASES}) == len(S.CASES)
    for c in S.CASES:
        assert c.covers, f"{c.name}: no exported name under test"
        assert c.compare, c.name
        assert set(c.sync) <= set(S.VARIANTS), c.name
        assert bool(c.sync) == bool(c.why), f"{c.name}: an inspect-class variant needs its reason (and only that needs one)"
        real = c.inputs("real")
        assert set(c.late) <= set(real) and c.late, c.name
    assert set(S.MISORDERED) <= set(S.BY_NAME)
    # part B: one owner of each kind the library has
    owners = {type(c).__name__ + ("/block" if getattr(c, "block", False) else "") for c in S.CASES if c.owner}
    assert owners == {"Spmv", "Spmm", "Trsv", "Trsv/block", "Sweeps", "Ilu0", "GaussSeidel", "Permute", "Spgemm"}
    # the forms the late-input test is to cover
    paths = {(c.form, c.env.get(S.T2)) for c in S.CASES if isinstance(c, S.Spmv)}
    assert {("transposed", "0"), ("csc", "0"), ("transposed", "1"), ("csc", "1"), ("scaled", None), ("int64", None),
            ("matrix_opt", None)} <= paths
    assert {c.alg for c in S.CASES if isinstance(c, S.Spmv)} >= {None, S._capi.SPMV_AUTO, S._capi.SPMV_VECTOR,
                                                                  S._capi.SPMV_ROWBLOCK, S._capi.SPMV_SLICED}


@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_generators(case):
    real, decoy = case.inputs("real"), case.inputs("decoy")
    assert set(real) == set(decoy)
    for k in real:
        assert np.shape(real[k]) == np.shape(decoy[k]), f"{k}: both input sets live in one buffer"
        if k not in case.late:
            assert np.array_equal(real[k], decoy[k]), f"{k} is never written late: one value"
    assert any(not np.array_equal(real[k], decoy[k], equal_nan=True) for k in case.late)
    want_r, want_d = case.expected(real), case.expected(decoy)
    for w in want_r + want_d:
        assert np.isfinite(np.asarray(w, np.complex128)).all(), "an expected result is not finite"
    # the decoys' result differs from the real one in every output element (multicolor_order: as a whole, see its docstring)
    assert case.separated(S.device_form(case, want_r), S.device_form(case, want_d))
    # the comparison passes the real result as the device would return it, and fails the decoys'
    assert case.violations(S.device_form(case, want_r), want_r) == []
    assert case.violations(S.device_form(case, want_d), want_r) != []
    if case.name in S.MISORDERED:      # part C compares with expected(decoy) as well: it must be exact too
        assert case.violations(S.device_form(case, want_d), want_d) == []


def test_exact_families_stay_exact_in_the_value_type():
    """Every sum of the shared operand is an integer the narrowest value type holds: the 16-bit cases compare bit for bit."""
    o = S.operand()
    A = S.sps.csr_matrix((o.values, o.colind, o.rowptr), shape=o.shape)
    assert (A @ o.x).max() < 256 and (A @ o.B).max() < 256          # bfloat16: 8 significant bits
    assert (A.T @ o.xt).max() < 2 ** 24
    # index arrays are valid for both input sets by construction: one structure
    assert o.colind.min() >= 0 and o.colind.max() < o.shape[1] and (np.diff(o.rowptr) >= 6).all()
