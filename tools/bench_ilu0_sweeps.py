"""ILU(0) by fixed-point sweeps (spblas_gfx950_ilu0_sweeps, csrc/ilu0.hip) against the exact, level-scheduled ilu0 of the SAME run,
fp32 and fp64, on the two matrices of tools/bench_ilu0.py (built by its functions):
  laplace7   the 7-point Laplacian on a --grid^3 cube in natural order (160^3 = 4 096 000 rows, 3 * grid - 2 levels);
  random9    --rows rows with the diagonal and 8 random columns spread over both triangles.
Protocol (that of tools/bench_ilu0.py): ilu0_inspect once; three warm-up calls of everything; then --rounds rounds alternating
the exact factor (out of place) and ilu0_sweeps at s = 1, 2, 3, 5, every figure --calls calls between two device events (one
synchronisation per figure and round); a round's figure is its time / calls.  Reported per case: median, min and max over the
rounds, and for each s
  |LU(s) - LU|_F / |LU|_F                on the device, at full size, LU the exact factor of the same run;
  |(A - L(s) U(s)) on the pattern|_F / |A|_F   on the HOST in float64 at a reduced size (--small-grid^3 / --small-rows rows, the
                                         same generators and type; scipy forms L(s) U(s)): the full-size product is not formed.
One sweep's time -- the slope between the smallest and the largest count that really ran, (t(5) - t(1)) / 4 where levels > 5,
beside t(1), which also holds the reset of the status word; none where the clamp leaves one count -- is set against the bytes a
sweep must move by the shapes alone, nnz x (4 + 2 sizeof(T)) + m x 8 (columns, A's values, the stored iterate; offsets and
diagonal positions; the gathers of pivots and pivot rows come on top), and against the device-to-device copy rate measured in
this run on a buffer of nnz values.
--resources FILE: the text of `hipcc ... -Rpass-analysis=kernel-resource-usage` for csrc/ilu0.hip; the sweep kernel's figures
are copied into the report.  Writes ilu0_sweeps_bench.json and ilu0_sweeps_bench.md into --out-dir and prints the JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import spblas_reference_amd as sp  # noqa: E402
from bench_ilu0 import kernel_resources, laplace7, random9, round_ms, stats  # noqa: E402

SWEEPS = (1, 2, 3, 5)


def copy_rate_gbs(nnz, dtype, dev, calls):
    src, dst = torch.rand(nnz, dtype=dtype, device=dev), torch.empty(nnz, dtype=dtype, device=dev)
    for _ in range(3):
        dst.copy_(src)
    ts = [round_ms(lambda: dst.copy_(src), calls) for _ in range(5)]
    return 2.0 * nnz * src.element_size() / (float(np.median(ts)) * 1e-3) / 1e9


def pattern_residuals(a, info_small):
    """|(A - L(s) U(s)) on the pattern|_F / |A|_F for s in SWEEPS and for the exact factor, on the host in float64."""
    import scipy.sparse as sps
    m, nnz = a.shape()[0], a.size()
    rp, ci = a.rowptr().cpu().numpy().astype(np.int64), a.colind().cpu().numpy()[:nnz].astype(np.int64)
    av = a.values().cpu().numpy()[:nnz].astype(np.float64)
    rows = np.repeat(np.arange(m), np.diff(rp))
    P = sps.csr_matrix((np.ones(nnz), ci, rp), shape=(m, m))
    lu = sp.csr_view(torch.empty_like(a.values()), a.rowptr(), a.colind(), (m, m), nnz)
    work = torch.empty_like(a.values())

    def residual():
        v = lu.values().cpu().numpy()[:nnz].astype(np.float64)
        low = ci < rows
        L = sps.csr_matrix((np.concatenate([v[low], np.ones(m)]), (np.concatenate([rows[low], np.arange(m)]),
                                                                   np.concatenate([ci[low], np.arange(m)]))), shape=(m, m))
        U = sps.csr_matrix((v[~low], (rows[~low], ci[~low])), shape=(m, m))
        R = (L @ U).multiply(P) - sps.csr_matrix((av, ci, rp), shape=(m, m))
        return float(np.sqrt(R.multiply(R).sum()) / np.linalg.norm(av))

    out = {}
    for s in SWEEPS:
        sp.ilu0_sweeps(info_small, a, lu, work, s)
        torch.cuda.synchronize()
        out[str(s)] = residual()
    sp.ilu0(info_small, a, lu)
    torch.cuda.synchronize()
    out["exact"] = residual()
    return out


def case(name, a, small, args, dev):
    dtype = a.values().dtype
    m, nnz = a.shape()[0], a.size()
    new_lu = lambda: sp.csr_view(torch.empty_like(a.values()), a.rowptr(), a.colind(), (m, m), nnz)
    lu, lus, work = new_lu(), new_lu(), torch.empty_like(a.values())
    info = sp.ilu0_inspect(a)

    def exact():
        sp.ilu0(info, a, lu)

    def swept(s):
        return lambda: sp.ilu0_sweeps(info, a, lus, work, s)

    for _ in range(3):
        exact()
        for s in SWEEPS:
            swept(s)()
    status = sp.ilu0_status(info)
    torch.cuda.synchronize()
    te, tsw = [], {s: [] for s in SWEEPS}
    for _ in range(args.rounds):
        te.append(round_ms(exact, args.calls))
        for s in SWEEPS:
            tsw[s].append(round_ms(swept(s), args.calls))
    exact()
    norm = float(torch.linalg.vector_norm(lu.values()[:nnz].double()))
    diffs = {}
    for s in SWEEPS:
        swept(s)()
        diffs[str(s)] = float(torch.linalg.vector_norm(lus.values()[:nnz].double() - lu.values()[:nnz].double())) / norm
    finite = bool(torch.isfinite(lus.values()[:nnz]).all())
    pi = info.state_.info()
    esz = a.values().element_size()
    sweep_bytes = nnz * (4 + 2 * esz) + m * 8
    med = {s: float(np.median(tsw[s])) for s in SWEEPS}
    # the slope between the smallest and the largest count that really ran (the call clamps s to max(1, levels - 1));
    # none where the clamp leaves one count or the slope is not positive: then no rate is reported
    ran = sorted({min(s, max(1, pi["levels"] - 1)) for s in SWEEPS})
    s_lo, s_hi = ran[0], ran[-1]
    t_of = {min(s, max(1, pi["levels"] - 1)): med[s] for s in reversed(SWEEPS)}
    slope = (t_of[s_hi] - t_of[s_lo]) / (s_hi - s_lo) if s_hi > s_lo else None
    one_sweep_ms = slope if slope is not None and slope > 0 else None
    copy = copy_rate_gbs(nnz, dtype, dev, args.calls)
    small_info = sp.ilu0_inspect(small)
    rec = {"matrix": name, "dtype": str(dtype).replace("torch.", ""), "m": m, "nnz": nnz, "levels": pi["levels"],
           "lanes_per_row": pi["lanes_per_row"], "status": status, "finite": finite, "exact_ms": stats(te),
           "sweeps_ms": {str(s): stats(tsw[s]) for s in SWEEPS},
           "sweeps_over_exact": {str(s): round(med[s] / float(np.median(te)), 3) for s in SWEEPS},
           "factor_difference": {k: float(f"{v:.3e}") for k, v in diffs.items()},
           "small": {"m": small.shape()[0], "nnz": small.size(), "levels": small_info.state_.info()["levels"]},
           "pattern_residual_small_fp64_host": {k: float(f"{v:.3e}") for k, v in pattern_residuals(small, small_info).items()},
           "one_sweep_ms": None if one_sweep_ms is None else round(one_sweep_ms, 4), "slope_between": [s_lo, s_hi],
           "first_sweep_call_ms": round(med[1], 4), "sweep_bytes": sweep_bytes,
           "sweep_gbs": None if one_sweep_ms is None else round(sweep_bytes / (one_sweep_ms * 1e-3) / 1e9, 1),
           "copy_gbs": round(copy, 1)}
    rec["sweep_over_copy_rate"] = None if one_sweep_ms is None else round(rec["sweep_gbs"] / rec["copy_gbs"], 3)
    return rec


def markdown(out):
    fmt = lambda t: f"{t['median']} ({t['min']} .. {t['max']})"
    lines = ["# ILU(0) by fixed-point sweeps against the exact, level-scheduled factor of the same run", "",
             f"Device: {out['device']}.  {out['rounds']} rounds alternating the exact `ilu0` and `ilu0_sweeps` at s = 1, 2, 3, 5, "
             f"{out['calls']} calls per figure between two device events; ms per call, median (min .. max) over the rounds.  "
             "Written by tools/bench_ilu0_sweeps.py.", "",
             "| matrix | type | rows | entries | levels | lanes per row | exact ilu0, ms | s = 1, ms | s = 2, ms | s = 3, ms | s = 5, ms | "
             "s = 1 / 2 / 3 / 5 over exact |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        lines.append(f"| {r['matrix']} | {r['dtype']} | {r['m']} | {r['nnz']} | {r['levels']} | {r['lanes_per_row']} | "
                     f"{fmt(r['exact_ms'])} | " + " | ".join(fmt(r["sweeps_ms"][str(s)]) for s in SWEEPS) + " | "
                     + " / ".join(str(r["sweeps_over_exact"][str(s)]) for s in SWEEPS) + " |")
    lines += ["", "How far the swept factor is from the exact one: ‖LU⁽ˢ⁾ − LU‖_F / ‖LU‖_F on the device at full size, and "
              "‖(A − L⁽ˢ⁾U⁽ˢ⁾) on the pattern‖_F / ‖A‖_F on the host in float64 at a reduced size (same generator and type; "
              "the last column is the exact factor's own residual there).", "",
              "| matrix | type | difference s = 1 | s = 2 | s = 3 | s = 5 | reduced size: rows (levels) | residual s = 1 | s = 2 | s = 3 | "
              "s = 5 | exact |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        d, p = r["factor_difference"], r["pattern_residual_small_fp64_host"]
        lines.append(f"| {r['matrix']} | {r['dtype']} | " + " | ".join(f"{d[str(s)]:.1e}" for s in SWEEPS)
                     + f" | {r['small']['m']} ({r['small']['levels']}) | " + " | ".join(f"{p[str(s)]:.1e}" for s in SWEEPS)
                     + f" | {p['exact']:.1e} |")
    lines += ["", "One sweep, the slope between the smallest and the largest sweep count that ran ((t(5) − t(1)) / 4 where levels > 5; — where the clamp leaves one count), over the bytes the shapes alone make it move (nnz × (4 + 2 sizeof T) + m × 8; the "
              "gathers of pivots and pivot rows come on top), beside the device-to-device copy rate of this run:", "",
              "| matrix | type | one sweep, ms | first call t(1), ms | bytes per sweep | GB/s | copy, GB/s | share of the copy rate |",
              "|---|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        dash = lambda v: "—" if v is None else v
        lines.append(f"| {r['matrix']} | {r['dtype']} | {dash(r['one_sweep_ms'])} | {r['first_sweep_call_ms']} | {r['sweep_bytes']} | "
                     f"{dash(r['sweep_gbs'])} | {r['copy_gbs']} | {dash(r['sweep_over_copy_rate'])} |")
    lines.append("")
    if out["kernel_resources"]:
        lines += ["Kernel resources (`-Rpass-analysis=kernel-resource-usage`, gfx950):", "",
                  "| kernel | VGPRs | SGPRs | LDS bytes per block | scratch bytes per lane | waves per SIMD |", "|---|---|---|---|---|---|"]
        lines += [f"| `{k['kernel']}` | {k['vgprs']} | {k['sgprs']} | {k['lds_bytes']} | {k['scratch_bytes']} | {k['waves_per_simd']} |"
                  for k in out["kernel_resources"]]
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=160)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--small-grid", type=int, default=40)
    ap.add_argument("--small-rows", type=int, default=64_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--dtypes", nargs="*", default=["float32", "float64"])
    ap.add_argument("--matrices", nargs="*", default=["laplace7", "random9"])
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ilu0_sweeps.py measures on the GPU: no device, no number"
    dev = torch.device("cuda:0")
    recs = []
    for name in args.matrices:
        for dn in args.dtypes:
            dtype = getattr(torch, dn)
            if name == "laplace7":
                a, small = laplace7(args.grid, dtype, dev), laplace7(args.small_grid, dtype, dev)
            else:
                a, small = random9(args.rows, dtype, dev), random9(args.small_rows, dtype, dev)
            recs.append(case(name, a, small, args, dev))
            print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
            del a, small
            torch.cuda.empty_cache()
    out = {"metric": "ilu0_sweeps_vs_exact_ilu0", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "calls": args.calls, "records": recs,
           "kernel_resources": [k for k in kernel_resources(args.resources) if "sweep" in k["kernel"]]}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "ilu0_sweeps_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(args.out_dir, "ilu0_sweeps_bench.md"), "w") as f:
        f.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
