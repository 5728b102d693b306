"""-m gpu: the ladders of tests/ladder_tt.py on the device -- the radix transpose and scale_kernel of csrc/transpose.hip bit for
bit against oracle.transpose / one IEEE multiply, and the level plan of csrc/sptrsv.hip (vector solve, and csrc/sptrsm.hip's
block of three columns on the same plan) on integer systems whose solution must come out EXACTLY, under the default plan,
Kahn's inspect, one launch per level group, a cooperative grid of 3 workgroups and a `narrow` limit above every level.  Each
test ends by comparing the set of rungs and paths it ran with the set it intended."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gpu_util as G
import ladder_tt as T
import spblas_reference_amd as sp
import tt_ladder_run as R
from test_gpu_sptrsv import check as sptrsv_check

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
VTS = ["f32", "f64"]

# ============================================================================================================ transpose
PASSES_OF_N = {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 65535: 2, 65536: 2, 65537: 3, 2 ** 24 - 1: 3, 2 ** 24: 3, 2 ** 24 + 1: 4}


@pytest.mark.parametrize("vt", VTS)
def test_transpose_column_ladder(gpu, vt):
    """Family 1: 1 / 2 / 3 / 4 passes (the pass count is a function of n alone: asserted through n), both layouts of the
    scratch sets, columns 0 and n - 1 in use; then four cases in which ONE byte of the column decides the order."""
    ran = {}
    for case in T.column_cases():
        if case.name.startswith("n"):
            assert case.passes == PASSES_OF_N[case.n] and {0, case.n - 1} <= set(case.colind.tolist())
        else:
            assert case.passes == 4
        R.run_transpose(case, vt)
        if case.n in (256, 65537, 2 ** 24 + 1):
            R.run_transpose(case, vt, off64=True)
        ran[case.name] = case.passes
    assert ran == {**{f"n{n}": p for n, p in PASSES_OF_N.items()}, **{f"byte{k}": 4 for k in range(4)}}


@pytest.mark.parametrize("off64", [False, True], ids=["offsets32", "offsets64"])
@pytest.mark.parametrize("vt", VTS)
def test_transpose_entry_and_row_ladders(gpu, vt, off64):
    """Families 2 and 3: entry counts around the tile, the rounds and the XCD remap's body / remainder; rows against tiles."""
    t = T.transpose_limits()
    ran = set()
    for case in T.entry_cases() + T.row_cases():
        R.run_transpose(case, vt, off64=off64)
        ran.add(case.name)
    tile = t["tile"]
    want = {f"nnz{z}" for z in list(range(1, 10)) + [1023, 1024, 1025, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile + 1]}
    want |= {f"nnz{k * tile + o}" for k in (7, 8, 9, 15, 16, 17) for o in (-1, 0, 1)}
    want |= {"nnz0", "m0", "m0_n0", "m1", "m1_empty", "start_at_tile", "span3", "carries", f"starts{t['mark_stride'] + 1}",
             f"starts{2 * t['mark_stride'] + 1}", "empties3000", "empties_tile_edge", "empties_trailing_full_tile"}
    assert ran == want


@pytest.mark.parametrize("vt", VTS)
def test_transpose_gap_and_bucket_ladders(gpu, vt):
    """Families 4 and 5: every class of gap of the row-offset fill as interior, leading and trailing gap, the long list as
    full as n admits; one bucket that takes everything, every digit once, duplicates across round / wave / tile edges."""
    ran = set()
    for case in T.gap_cases() + T.bucket_cases():
        R.run_transpose(case, vt)
        ran.add(case.name)
    assert ran == {f"gap{g}" for g in T.GAP_LENS} | {"long_full", "long_few", "one_column", "digits_once",
                                                     "digits_once_two_passes", "duplicates_on_edges"}


@pytest.mark.parametrize("vt", VTS)
def test_transpose_alignment_ladder(gpu, vt):
    """Family 6: colind, values and the three output arrays shifted by 0 ... 3 elements -- all together and one at a time."""
    case = T.alignment_case()
    ref = None
    ran = set()
    for shifts in T.ALIGN_SHIFTS:
        ref = R.run_transpose(case, vt, shifts=shifts, ref=ref)
        ran.add(shifts)
    assert len(ran) == 4 + 5 * 3 and {(s,) * 5 for s in range(4)} <= ran


@pytest.mark.parametrize("vt", VTS)
def test_transpose_state_between_calls(gpu, vt):
    """Family 7, on the thread's one handle: four passes (both scratch sets), then one tile in one pass, then long gaps, then
    none; each case twice in a row, and the whole sequence twice."""
    cases = T.state_cases()
    assert [c.passes for c in cases] == [4, 1, 2, 2]
    refs = [None] * len(cases)
    ran = []
    for _ in range(2):
        for i, case in enumerate(cases):
            for _ in range(2):
                refs[i] = R.run_transpose(case, vt, ref=refs[i])
                ran.append(case.name)
    assert ran == [c.name for c in cases for _ in range(2)] * 2


CHILD_LIMIT_S = 300


def test_transpose_ladders_without_the_xcd_remap(gpu):
    """SPBLAS_GFX950_TRANSPOSE_XCD=0 is read once per process: ONE child runs families 2 and 3 under it.  On a time limit or
    a signal the test fails and starts nothing else."""
    env = dict(os.environ)
    env["SPBLAS_GFX950_TRANSPOSE_XCD"] = "0"
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "tt_ladder_worker.py")], env=env, capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        raise AssertionError("SPBLAS_GFX950_TRANSPOSE_XCD=0: the child process ran into its time limit")
    assert p.returncode == 0, f"SPBLAS_GFX950_TRANSPOSE_XCD=0: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    n_cases = len(T.entry_cases()) + len(T.row_cases())
    assert p.stdout.strip().splitlines()[-1] == f"compared {2 * n_cases} cases with the remap off"


# ================================================================================================================ scale
def test_scale_ladder(gpu):
    """scale_kernel: head, vector body, tail and the capped grid; the whole base tensor is compared, so the elements in front
    of and behind the view must be untouched."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t = T.transpose_limits()
    cases = T.scale_cases(cus)
    ran = set()
    for vt, n, off in cases:
        R.run_scale(vt, n, off)
        ran.add((vt, n, off))
    want = set()
    for vt, per in (("f32", t["scale_per_f32"]), ("f64", t["scale_per_f64"])):
        full = cus * t["scale_blocks_per_cu"] * t["scale_block"] * per
        want |= {(vt, n, off) for n in range(71) for off in range(5)}
        want |= {(vt, n, off) for n in (full - 1, full, full + 1, full + 5, 2 * full + 3) for off in (0, 1)}
    assert ran == want and len(cases) == len(want)


# ===================================================================================================== triangular solve
def _run_random(sysm, vt):
    """The same structure with random values under a dominant diagonal, through test_gpu_sptrsv.check unchanged."""
    M = T.as_scipy(sysm, sysm.random_values)
    b = np.random.default_rng(sysm.m).random(sysm.m) + 0.5
    sptrsv_check(M, b, sysm.upper, sysm.unit, R.NUMPY_OF[vt])


BLOCKS = (("R", "R"), ("L", "L"), ("R", "L"))


@pytest.mark.parametrize("mode", ["default", "kahn", "coop0", "grid3"])
@pytest.mark.parametrize("unit", [False, True], ids=["explicit", "unit"])
@pytest.mark.parametrize("upper", [False, True], ids=["lower", "upper"])
@pytest.mark.parametrize("lanes", [4, 8, 16, 64])
def test_trsv_row_shape_ladder(gpu, monkeypatch, lanes, upper, unit, mode):
    """C1: strict counts 0 ... 2G + 2, 3G - 1 ... 3G + 1 and 300; the diagonal first, last, at G - 1, G, 2G - 1, 2G, absent (unit),
    stored twice with the pair in (c0, c1), (c1, loop), (loop, loop).  Under a grid of 3 workgroups the wide level is wider than
    the pipelined pass of the 64-lane kernel, so shapes also run through the plain passes behind it.  The lower
    systems also run as a block of three columns (csrc/sptrsm.hip on the same plan), in both layouts."""
    sysm = T.shape_system(lanes, upper, unit)
    names = {s.name for s in T.row_shapes(lanes, unit)}
    narrow = T.trsv_limits()["narrow"]
    widths, k = T.shape_widths(lanes, unit)
    assert sysm.widths == widths and max(widths[1:1 + k]) < narrow <= widths[1 + k]
    for lo, hi in ((1, 1 + k), (1 + k, 2 + k), (2 + k, 2 + 2 * k)):   # the first narrow run, the wide level, the last run
        assert set(sysm.shape_of[(sysm.level >= lo) & (sysm.level < hi)]) == names, f"levels {lo} ... {hi - 1} miss a shape"
    if mode == "grid3" and lanes == 64:
        assert widths[1 + k] > T.pipelined_pass(3, lanes)
    blocks = BLOCKS if mode in ("default", "coop0") and not upper else ()
    ran = set()
    for vt in VTS:
        a, A, info = R.inspect(sysm, vt, mode, monkeypatch)
        assert info.state_.info()["lanes_per_row"] == lanes
        R.solve_exact(sysm, vt, A, info)
        ran.add((vt, "exact"))
        for block in blocks:
            R.solve_exact(sysm, vt, A, info, block=block)
            ran.add((vt, block))
    if mode == "default":
        _run_random(sysm, "f32" if upper else "f64")
        ran.add("random")
    assert ran == {(vt, w) for vt in VTS for w in ("exact",) + blocks} | ({"random"} if mode == "default" else set())


def test_trsv_mean_row_length_ladder(gpu, monkeypatch):
    """Lanes per row step where the mean row length EXCEEDS 6 / 24 / 96: nnz = limit * m entries take the lower count, one
    entry more the higher."""
    ran = {}
    for limit, extra, lanes, sysm in T.mean_cases():
        assert sysm.nnz == limit * sysm.m + extra
        for vt in VTS:
            a, A, info = R.inspect(sysm, vt, "default", monkeypatch)
            R.solve_exact(sysm, vt, A, info)
        ran[(limit, extra)] = info.state_.info()["lanes_per_row"]
    assert ran == {(6, 0): 4, (6, 1): 8, (24, 0): 8, (24, 1): 16, (96, 0): 16, (96, 1): 64}


@pytest.mark.parametrize("mode", ["grid3", "kahn", "coop0", "narrow100000"])
@pytest.mark.parametrize("lanes", [4, 8, 16, 64])
def test_trsv_level_width_ladder_small_grid(gpu, monkeypatch, lanes, mode):
    """C2 under SPBLAS_GFX950_TRSV_COOP_GRID=3 (and the same system through the other plans; a `narrow` limit of 100 000 makes
    one group of everything)."""
    t = T.trsv_limits()
    upper, unit = lanes in (8, 64), lanes in (16, 64)
    sysm, P = T.width_system(lanes, 3, upper, unit)
    assert P == 3 * (t["coop_threads"] // lanes) * t["slots"][lanes]
    assert {1, 2, 3, 4, 5, t["narrow"] - 1, t["narrow"], t["narrow"] + 1, P - 1, P, P + 1, 2 * P + 1} <= set(sysm.widths)
    ran = set()
    for vt in VTS:
        a, A, info = R.inspect(sysm, vt, mode, monkeypatch)
        pi = info.state_.info()
        if mode == "narrow100000":
            assert pi["launches_per_solve"] == 1 and max(sysm.widths) < 100000
        if mode == "coop0":
            assert pi["launches_per_solve"] == len(T.groups_of(sysm.widths, t["narrow"])) > 1
        if mode == "grid3" and not R.hsa_tool_loaded():
            assert pi["launches_per_solve"] == 1
        R.solve_exact(sysm, vt, A, info)
        R.solve_exact(sysm, vt, A, info)                            # a second solve on the plan: the control words are reset
        ran.add(vt)
    if mode == "grid3":
        _run_random(sysm, "f32")
    assert ran == set(VTS)


@pytest.mark.parametrize("lanes", [16, 64])
def test_trsv_level_width_ladder_default_grid(gpu, monkeypatch, lanes):
    """C2 at the default grid (one workgroup per CU): P from the device's CU count, for 64 and 16 lanes per row."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sysm, P = T.width_system(lanes, cus)
    assert {P - 1, P, P + 1, 2 * P + 1} <= set(sysm.widths)
    ran = set()
    for vt in VTS:
        a, A, info = R.inspect(sysm, vt, "default", monkeypatch)
        if not R.hsa_tool_loaded():
            assert info.state_.info()["launches_per_solve"] == 1
        R.solve_exact(sysm, vt, A, info)
        ran.add(vt)
    assert ran == set(VTS)


@pytest.mark.parametrize("mode", ["default", "kahn", "coop0"])
def test_trsv_level_sequences(gpu, monkeypatch, mode):
    """C3: 1 ... 5 levels (the pipeline's prologue runs past the last level), every transition between a narrow and a wide
    level, a narrow run as the first and as the last group."""
    t = T.trsv_limits()
    assert T.NARROW_W < t["narrow"] <= T.WIDE_W
    ran = set()
    for i, widths in enumerate(T.SEQUENCES):
        sysm = T.sequence_system(i)
        for vt in VTS:
            a, A, info = R.inspect(sysm, vt, mode, monkeypatch)
            R.solve_exact(sysm, vt, A, info)
        ran.add(tuple(widths))
    assert ran == {tuple(w) for w in T.SEQUENCES} and {len(w) for w in T.SEQUENCES} == {1, 2, 3, 4, 5}
    pairs = {(a >= t["narrow"], b >= t["narrow"]) for w in T.SEQUENCES for a, b in zip(w, w[1:])}
    assert pairs == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize("mode", ["default", "kahn", "coop0"])
def test_trsv_long_narrow_runs_and_chains(gpu, monkeypatch, mode):
    """C3: a narrow run of 4 096 levels next to one wide level keeps the cooperative launch (ONE launch per solve), one of 4 097
    switches it off (one launch per group); chains of 4 095 ... 4 098 levels straddle the inspect's LDS histogram."""
    t = T.trsv_limits()
    run, hist = t["max_run"], t["hist_levels"]
    ran = {}
    for i, (name, widths) in enumerate(T.long_run_cases()):
        sysm = T.long_run_system(i)
        vt = VTS[i % 2]
        a, A, info = R.inspect(sysm, vt, mode, monkeypatch)
        pi = info.state_.info()
        assert pi["levels"] == len(widths)
        R.solve_exact(sysm, vt, A, info)
        ran[name] = pi["launches_per_solve"]
    coop = mode != "coop0" and not R.hsa_tool_loaded()
    assert ran == {f"wide_then_{run}": 1 if coop else 2, f"wide_then_{run + 1}": 2, f"{run}_then_wide": 1 if coop else 2,
                   f"{run + 1}_then_wide": 2, **{f"chain{k}": 1 for k in (hist - 1, hist, hist + 1, hist + 2)}}


def test_trsv_kahn_limits(gpu, monkeypatch):
    """C4 under SPBLAS_GFX950_TRSV_KAHN=1: frontiers of 2 047 / 2 048 / 2 049 rows, 15 / 16 / 17 wide frontiers in a row (batches
    of 16 launches), m = 1, 31, 32, 33 (32 rows per workgroup) and m around 512 x 32 (the advance grid's cap)."""
    t = T.trsv_limits()
    batch, edge = t["kahn_batch"], t["kahn_rows_per_block"] * t["kahn_max_blocks"]
    ran = set()
    for i, (name, widths) in enumerate(T.kahn_cases()):
        sysm = T.kahn_system(i)
        assert sysm.m == sum(widths)
        vt = VTS[i % 2]
        a, A, info = R.inspect(sysm, vt, "kahn", monkeypatch)
        R.solve_exact(sysm, vt, A, info)
        ran.add(name)
    assert ran == {"frontiers", f"wide{batch - 1}", f"wide{batch}", f"wide{batch + 1}", "m1", "m31", "m32", "m33",
                   f"m{edge - 1}", f"m{edge}", f"m{edge + 1}"}


@pytest.mark.parametrize("upper", [False, True], ids=["lower", "upper"])
def test_trsv_ladder_system_in_a_graph(gpu, monkeypatch, upper):
    """C5: a solve of a ladder system recorded into a graph (the first solve runs outside the capture, as the API requires)
    and replayed on new right-hand sides: x_true times 1 and times -2, exactly."""
    sysm = T.shape_system(8, upper, False)
    a, A, info = R.inspect(sysm, "f32", "default", monkeypatch)
    x = R.solve_exact(sysm, "f32", A, info)
    uplo, diag = R.tags(upper, False)
    b = G.dev(sysm.b.astype(np.float32))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sp.triangular_solve(info, A, uplo, diag, b, x)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sp.triangular_solve(info, A, uplo, diag, b, x)
    ran = []
    for f in (1.0, -2.0):
        b.copy_(G.dev((sysm.b * f).astype(np.float32)))
        x.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        got, want = G.host(x), (sysm.x_true * f).astype(np.float32)
        assert np.array_equal(got, want), f"replay with b * {f}: {np.count_nonzero(got != want)} rows differ"
        ran.append(f)
    assert ran == [1.0, -2.0]
