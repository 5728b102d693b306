"""The block ladder of the SpMM panel / band path (tests/ladder_mm.py) proves itself on the host: every family's blocks are
what their specification claims under the restated probe, its fp64 reference equals the oracle's SpMM, the host model of the
kernels equals the reference -- and three mutations of that model each fail a rung, so the rungs discriminate."""
import numpy as np
import pytest

import ladder_mm as M
from oracle import oracle

E = M.E


def test_constants_parsed_from_the_source_are_the_ones_the_families_were_written_for():
    c = M.constants()
    assert (c["MM_RB"], c["MM_KT"], c["MM_MAXT"], c["MM_NP"], c["EB"]) == (32, 64, 16, 128, 8)
    assert c["ADMIT_DIV"] == 12 and c["MIN_DEFAULT"] == 170
    assert (c["CH_DEFAULT"], c["CH_MIN"], c["CH_MAX"]) == (128, 64, 312)
    assert c["LDS_BYTES"] == 160 * 1024 and c["MM_DENSE_CH"] == 248
    # the entry loop's LDS at the clamp is exactly what a workgroup can have; the matrix-core kernel's at its row cap leaves
    # 4 KiB for that kernel's static LDS
    assert (c["MM_DENSE_CH"] * c["MM_NP"] + ((c["MM_DENSE_CH"] + 31) & ~31) * c["MM_RB"]) * 4 + 4096 == c["LDS_BYTES"]
    assert c["CH_MAX"] * c["MM_NP"] * 4 + 8 * 512 == c["LDS_BYTES"]
    # the row lengths sit around the 8-entry batches and the 64-entry reloads of the entry loop
    assert {c["EB"] - 1, c["EB"], c["EB"] + 1, 63, 64, 65, 127, 128, 129} <= set(M.ROW_LENGTHS)
    assert 87 in M.PAIR_DISTANCES and {63, 64, 65} <= set(M.PAIR_DISTANCES)


def test_knobs_restate_the_inspect():
    assert M.knobs({}) == {"min_per_tile": 170, "band": 1, "band_ch": 128, "band_waves": 8, "dense_pm": 1001}
    assert M.knobs({E + "PANEL_MIN": "64", E + "BAND_CH": "20"})["band_ch"] == 64
    assert M.knobs({E + "BAND_CH": "400"})["band_ch"] == 312
    assert M.knobs({E + "BAND_CH": "312", E + "BAND_WAVES": "16"})["band_ch"] == 304     # 304 * 512 + 16 * 512 = 160 KiB
    assert M.knobs({E + "BAND_CH": "312", E + "BAND_WAVES": "4"})["band_ch"] == 312
    assert M.knobs({E + "BAND": "0", E + "BAND_DENSE": "0"})["dense_pm"] == 1001
    assert M.knobs({E + "BAND_DENSE": "250"})["dense_pm"] == 250
    assert [M.group_size(ch) for ch in (64, 100, 127, 128, 255, 256, 304, 312)] == [1, 1, 1, 2, 3, 4, 4, 4]


def claim_failures(f, env, mutation=None):
    kind, nt, tiles, win, _ = M.probe_family(f, env, mutation)
    ch = M.knobs(env)["band_ch"]
    bad = []
    for b, cl in f.claims.items():
        W = int(win[b, 1]) - int(win[b, 0]) + 1
        got = {"kind": int(kind[b]), "nt": int(nt[b]), "W": W, "branch": "single" if W - 1 < ch else "wide"}
        for key, want in cl.items():
            if key == "branch" and kind[b] != 1:
                continue
            if got[key] != want:
                bad.append(f"{f.name} block {b}: {key} is {got[key]}, the specification says {want}")
    return bad


def value_failures(f, env, mutation=None, n=3):
    values, B, _ = M.exact_data(f)
    ref, _ = M.reference(f, values, B[:, :n])
    got = M.host_model(f, values, B[:, :n], env, mutation)
    rows = np.flatnonzero(~(got == ref).all(axis=1))
    return [f"{f.name}: the model differs from the reference in rows {rows[:6].tolist()} (blocks {sorted(set(rows // 32))[:6]})"] \
        if len(rows) else []


@pytest.mark.parametrize("name", list(M.GROUPS))
def test_every_block_is_what_its_specification_claims(name):
    fams = M.group(name)
    assert fams and all(f.claims for f in fams)
    for f in fams:
        assert not claim_failures(f, f.env)
    if name in ("window", "wide"):     # laid around the chunk each selection really stages
        for sel in M.SELECTIONS:
            if sel not in ("band_mfma", "tiles"):          # (their blocks go to other kernels: no branch to claim)
                for f in M.group(name, sel):
                    assert not claim_failures(f, M.env_of(f, sel)), sel


def test_the_families_hold_the_rungs_the_ladder_names():
    # admission: both sides of min_per_tile * nt for every tile count, at both thresholds; overflow; cheap reject
    for mpt in (170, 64):
        f = M.fam_admission(mpt)
        kind, nt, _, _, _ = M.probe_family(f, f.env)
        cnt = np.add.reduceat(np.diff(f.rowptr), np.arange(0, f.m, 32))
        for t in range(1, 17):
            assert {int(x) - mpt * t for x in cnt[(nt == t)]} >= {0, 1} and (kind[(nt == t) & (cnt >= mpt * t)] == 1).all()
            assert ((cnt == mpt * t - 1) & (kind == 0)).any()
        assert (nt == 17).sum() == 1 and ((cnt == mpt - 1) & (nt == 0)).any()
    # window against chunk: W on both sides of every chunk, every kmin mod 4, column 0, the last column for three k mod 64
    seen = set()
    for f in M.group("window"):
        ch = M.knobs(f.env)["band_ch"]
        kind, _, _, win, _ = M.probe_family(f, f.env)
        q = kind == 1
        W = win[q, 1] - win[q, 0] + 1
        assert set(W.tolist()) == {ch - 1, ch, ch + 1}
        for w_ in (ch - 1, ch, ch + 1):
            assert {int(x) % 4 for x in win[q, 0][W == w_]} == {0, 1, 2, 3} and (win[q, 0][W == w_] == 0).any()
            assert (win[q, 1][W == w_] == f.k - 1).any()
        seen.add((ch, f.k % 64))
    assert {ch for ch, _ in seen} == {64, 100, 128, 312} and {km for _, km in seen} == {0, 1, 63}
    # wide branch: tile counts around every group size
    for f in M.group("wide"):
        ch = M.knobs(f.env)["band_ch"]
        G = M.group_size(ch)
        kind, nt, _, win, _ = M.probe_family(f, f.env)
        wide = (kind == 1) & (win[:, 1] - win[:, 0] >= ch)
        assert {n_ for n_ in (G - 1, G, G + 1, 2 * G - 1, 2 * G + 1, 16) if n_ >= 2} <= set(nt[wide].tolist()), f.name
    assert {M.group_size(M.knobs(f.env)["band_ch"]) for f in M.group("wide")} == {1, 2, 4}
    # row shapes: every length on every row position
    for f in M.group("row_shapes"):
        lens = np.diff(f.rowptr).reshape(-1, 32)
        for r in range(32):
            assert set(M.ROW_LENGTHS) <= set(lens[:, r].tolist())
        assert ((lens[:, :31] == 0).all(axis=1) & (lens[:, 31] > 0)).any() and ((lens[:, 8:16] == 0).all(axis=1) & (lens[:, 0] > 0)).any()
    # dense rule: the contraction's step counts -- zero, one, two rounds of the 8-step unroll, with and without a tail
    f = M.fam_dense(128, 250)
    kind, _, _, win, _ = M.probe_family(f, f.env)
    Wp = ((win[kind == 2, 1] - win[kind == 2, 0] + 1 + 3) & ~3)
    assert {4, 28, 32, 36, 60, 64, 68, 128} <= set(Wp.tolist())
    assert (100 + 31) & ~31 == 128 and M.fam_dense(100, 250) in M.group("dense")   # a chunk whose A tile stride differs from it
    # partial last block and lists
    assert [f.m % 32 for f in M.group("partial")] == [1, 2, 4, 8, 31, 31] and M.group("partial")[-1].m == 31
    nq = [int((M.probe_family(f, f.env)[0] > 0).sum()) for f in M.group("lists")[:20]]
    assert nq == list(range(1, 18)) + [63, 64, 65]
    ap, ap1 = M.fam_all_panel(False), M.fam_all_panel(True)
    assert (M.probe_family(ap, ap.env)[0] > 0).all() and (M.probe_family(ap1, ap1.env)[0] == 0).sum() == 1
    assert [len(M.probe_family(f, f.env)[0]) for f in M.group("nblk")] == [255, 256, 257, 2047, 2048, 2049]


@pytest.mark.parametrize("name", list(M.GROUPS))
def test_reference_equals_the_oracle_and_the_host_model_equals_the_reference(name):
    for f in M.group(name):
        values, B, C0 = M.exact_data(f)
        ref, _ = M.reference(f, values, B[:, :5])
        got = oracle.spmm(f.shape, f.rowptr, f.colind, values.astype(np.float64), B[:, :5])
        assert np.array_equal(got, ref), f.name
        full, _ = M.reference(f, values, B[:, :5], -2.0, 0.5, C0[:, :5])
        assert np.array_equal(full, -2.0 * got + 0.5 * C0[:, :5])
        if f.m <= 10000:              # (the model walks rows in Python)
            for sel in M.SELECTIONS:
                assert not value_failures(f, M.env_of(f, sel)), sel


def test_reference_multiplies_stored_entries_only():
    f = M.fam_partial(4)
    values, B, _ = M.exact_data(f)
    B = B[:, :3].copy()
    col = int(f.colind[f.rowptr[0]])
    B[col, 1] = np.inf
    ref, _ = M.reference(f, values, B)
    hit = np.array([(f.colind[f.rowptr[r]:f.rowptr[r + 1]] == col).any() for r in range(f.m)])
    assert np.isfinite(ref[~hit]).all() and not np.isfinite(ref[hit, 1]).any() and hit.any() and not hit.all()


MUTATIONS = {"later_only": "keep only the later entry of a repeated pair",
             "le_ch": "<= CH instead of < CH for the branch switch",
             "w_not_wp": "W instead of Wp in the dense rule"}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_a_mutated_host_model_fails_a_rung(mutation):
    fams = M.group("window") + M.group("dense") + M.group("repeated")
    clean = [x for f in fams for x in claim_failures(f, f.env) + value_failures(f, f.env)]
    assert not clean
    bad = [x for f in fams for x in claim_failures(f, f.env, mutation) + value_failures(f, f.env, mutation)]
    assert bad, f"no rung notices: {MUTATIONS[mutation]}"
