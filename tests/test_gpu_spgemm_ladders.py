"""-m gpu: the SpGEMM / add ladder of tests/ladder.py on the device (csrc/spgemm.hip: three- and four-argument products and
add()).  Every family (lanes per B row x A's mean row length) x {fp32, fp64} x {EXACT, RANDOM}: the symbolic pass, five numeric
passes on the one state, structure exact, every entry of C compared (EXACT: bit for bit), and the row counts of
spgemm_state_t.info() EQUAL to what the classification rule restated in ladder.classify gives.  Knobs the library reads once
per process run in a fresh child each, one at a time; after a child that died nothing more is started."""
import os
import subprocess
import sys

import pytest

import ladder as L
import spg_ladder_run as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FAMILIES = L.spg_families()
FAM_IDS = [f"sub{s}_a{a}" for s, a in FAMILIES]
VTS = ["f32", "f64"]
DATA = ["EXACT", "RANDOM"]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("vt", VTS)
@pytest.mark.parametrize("fam", FAMILIES, ids=FAM_IDS)
def test_three_argument_ladder(gpu, fam, vt, data):
    assert R.run_product(R.family_case(*fam), vt, data == "EXACT", False) > 0


@pytest.mark.parametrize("reuse", ["2", "0"])
@pytest.mark.parametrize("vt", VTS)
@pytest.mark.parametrize("fam", FAMILIES, ids=FAM_IDS)
def test_three_argument_ladder_recording_first_or_never(gpu, monkeypatch, fam, vt, reuse):
    monkeypatch.setenv("SPBLAS_GFX950_SPGEMM_REUSE", reuse)
    R.run_product(R.family_case(*fam), vt, True, False)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("vt", VTS)
@pytest.mark.parametrize("fam", FAMILIES, ids=FAM_IDS)
def test_four_argument_ladder(gpu, fam, vt, data):
    R.run_product(R.family_case(*fam), vt, data == "EXACT", True)


@pytest.mark.parametrize("vt", VTS)
@pytest.mark.parametrize("fam", FAMILIES, ids=FAM_IDS)
def test_four_argument_ladder_without_sortable_rows(gpu, monkeypatch, fam, vt):
    """SPBLAS_GFX950_SPG_DIRECT_ADD=0: the rows with an addend hash (256 products + 64 addend entries are a row of bin 3), and
    the fills go by rank from the third on."""
    monkeypatch.setenv("SPBLAS_GFX950_SPG_DIRECT_ADD", "0")
    R.run_product(R.family_case(*fam), vt, True, True, classify_kw={"direct_add": False})


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("vt", VTS)
@pytest.mark.parametrize("fam", FAMILIES, ids=FAM_IDS)
def test_add_ladder(gpu, fam, vt, data):
    R.run_add(R.family_add_case(*fam), vt, data == "EXACT")


@pytest.mark.parametrize("fam", FAMILIES, ids=FAM_IDS)
def test_ladder_without_b_row_descriptors(gpu, monkeypatch, fam):
    """SPBLAS_GFX950_SPG_ADESC=0: the kernels look B's rows up themselves, and no row is sortable."""
    monkeypatch.setenv("SPBLAS_GFX950_SPG_ADESC", "0")
    for addend in (False, True):
        R.run_product(R.family_case(*fam), "f32", True, addend, passes=3, classify_kw={"adesc": False})


@pytest.mark.parametrize("n", L.SPG_NARROW_NS)
def test_narrow_c_in_every_bin(gpu, n):
    case = R.Case(f"narrow{n}", *L.spg_narrow(n))
    for vt in VTS:
        for addend in (False, True):
            R.run_product(case, vt, True, addend, passes=3)
    other = L.spg_narrow(n, seed=67)                               # (the same rows, other columns in the addend)
    add_case = R.Case(f"narrow{n}_add", case.dr, case.dc, None, None, other[4], other[5], (case.shape[0], n, n))
    R.run_add(add_case, "f32", True, passes=3)


def test_widest_c_the_abi_accepts(gpu):
    """n = 2^31 - 1, columns 0, 2^30 and n - 1 in use.  No dense-bin row: that bin allocates n values per workgroup."""
    arrays = L.spg_narrow(L.SPG_N_MAX, dense=False)
    case = R.Case("widest", *arrays)
    for addend in (False, True):
        pred = L.predicted_info(case.ar, case.ac, case.br, case.dr if addend else None)
        assert pred["dense_rows"] == 0, "the widest matrix must keep out of the dense bin"
    assert {0, 2 ** 30, L.SPG_N_MAX - 1} <= set(case.bc.tolist())
    for vt in VTS:
        for addend in (False, True):
            R.run_product(case, vt, True, addend, passes=3)


@pytest.mark.parametrize("m", L.SPG_ROW_COUNTS)
def test_row_count_ladder(gpu, m):
    case = R.Case(f"rows{m}", *L.spg_row_count_matrix(m))
    for addend in (False, True):
        R.run_product(case, "f32", True, addend, passes=3)


@pytest.mark.parametrize("total", [0, 1, 3, 4, 5])
def test_b_with_a_handful_of_entries(gpu, total):
    case = R.Case(f"tiny_b{total}", *L.spg_tiny_b(total))
    for addend in (False, True):
        R.run_product(case, "f64", True, addend, passes=3)


# ------------------------------------------------------------------------------------------------------ child processes
KNOBS = [("SPBLAS_GFX950_SPG_DIRECT", "0"), ("SPBLAS_GFX950_SPG_PACK", "0"), ("SPBLAS_GFX950_SPG_PACK", "1"),
         ("SPBLAS_GFX950_SPG_RANKED_TPR", "16"), ("SPBLAS_GFX950_SPG_RANKED_TPR", "32"), ("SPBLAS_GFX950_SPG_RANKED_TPR", "64"),
         ("SPBLAS_GFX950_SPG_RANKED_TPR1", "8"), ("SPBLAS_GFX950_SPG_RANKED_TPR1", "16")]
CHILD_LIMIT_S = 420
_died = []          # why a child ended by a signal or its time limit: nothing more is started on the card after that


@pytest.mark.parametrize("knob", KNOBS, ids=[f"{k[len('SPBLAS_GFX950_'):]}={v}" for k, v in KNOBS])
def test_exact_ladders_under_a_knob_read_once_per_process(gpu, knob):
    if _died:
        pytest.skip(f"an earlier child process of this module {_died[0]}: nothing more is started on the card")
    env = dict(os.environ)
    env[knob[0]] = knob[1]
    vts = "f32" if knob[0].endswith("SPG_PACK") else "f32,f64"       # (B is packed for fp32 fills only)
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "spg_ladder_worker.py"), vts], env=env, capture_output=True,
                           text=True, timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        _died.append(f"ran into its time limit of {CHILD_LIMIT_S} s ({knob[0]}={knob[1]})")
        raise AssertionError(f"{knob[0]}={knob[1]}: the child process ran into its time limit")
    if p.returncode < 0:
        _died.append(f"ended by signal {-p.returncode} ({knob[0]}={knob[1]})")
    assert p.returncode == 0, f"{knob[0]}={knob[1]}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    assert p.stdout.strip().splitlines()[-1].startswith("compared ")
