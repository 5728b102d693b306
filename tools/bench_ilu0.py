"""ILU(0) against what it enables: one factor call (csrc/ilu0.hip) next to one lower-unit plus one upper-explicit vector solve on
its result (csrc/sptrsv.hip), fp32 and fp64.

Matrices (built on the device, rows sorted, diagonal stored, diagonally dominant values):
  laplace7   the 7-point Laplacian on a --grid^3 cube in natural order (160^3 = 4 096 000 rows): the level sets are the
             hyperplanes i + j + k = const, 3 * grid - 2 of them;
  random9    --rows rows with the diagonal and 8 random columns spread over both triangles (repeats dropped).
Protocol: ilu0_inspect and the two triangular_solve_inspect calls once; three warm-up calls of each; then --rounds rounds
alternating (a) one factor (out of place: the copy of A's values is part of the call) and (b) the solve pair in this process,
every round --calls calls between two device events (one synchronisation per round); a round's figure is its time / calls.
Reported per case: median, min and max over the rounds of both, the ratio of the medians, levels, launches per factor, lanes
per row and what ilu0_status says (correctness is the test suite's business: tests/test_gpu_ilu0.py).
--resources FILE: the text of `hipcc ... -Rpass-analysis=kernel-resource-usage` for csrc/ilu0.hip; its register / LDS figures
are copied into the report.
Writes ilu0_bench.json and ilu0_bench.md into --out-dir and prints the JSON line."""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import spblas_reference_amd as sp  # noqa: E402


def laplace7(g, dtype, dev):
    n = g * g * g
    i = torch.arange(n, device=dev, dtype=torch.int64)
    x, y, z = i % g, (i // g) % g, i // (g * g)
    cand = [(i - g * g, z > 0), (i - g, y > 0), (i - 1, x > 0), (i, torch.ones_like(x, dtype=torch.bool)), (i + 1, x < g - 1),
            (i + g, y < g - 1), (i + g * g, z < g - 1)]
    cols = torch.stack([c for c, _ in cand], dim=1)
    keep = torch.stack([k for _, k in cand], dim=1)
    vals = torch.full(cols.shape, -1.0, dtype=dtype, device=dev)
    vals[:, 3] = 6.0 + 0.25 * torch.rand(n, dtype=dtype, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    rp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rp[1:] = keep.sum(dim=1).cumsum(0)
    return sp.csr_view(vals[keep].contiguous(), rp.int(), cols[keep].int().contiguous(), (n, n), int(rp[-1]))


def random9(m, dtype, dev, k=8):
    gen = torch.Generator(device=dev).manual_seed(2)
    rows = torch.arange(m, device=dev, dtype=torch.int64)
    cols = (torch.rand((m, k), device=dev, generator=gen, dtype=torch.float64) * m).long().clamp_(max=m - 1)
    cols = torch.cat([cols, rows[:, None]], dim=1).sort(dim=1).values
    keep = torch.ones_like(cols, dtype=torch.bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    vals = (torch.rand(cols.shape, device=dev, generator=gen, dtype=dtype) - 0.5)
    vals = torch.where(cols == rows[:, None], torch.full_like(vals, float(k)), vals)
    rp = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    rp[1:] = keep.sum(dim=1).cumsum(0)
    return sp.csr_view(vals[keep].contiguous(), rp.int(), cols[keep].int().contiguous(), (m, m), int(rp[-1]))


def round_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def stats(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(float(min(ts)), 4), "max": round(float(max(ts)), 4)}


def case(name, a, args, dev):
    dtype = a.values().dtype
    m, nnz = a.shape()[0], a.size()
    lu = sp.csr_view(torch.empty_like(a.values()), a.rowptr(), a.colind(), (m, m), nnz)
    b = torch.rand(m, dtype=dtype, device=dev)
    y, x = torch.empty_like(b), torch.empty_like(b)
    info = sp.ilu0_inspect(a)
    lo = sp.triangular_solve_inspect(lu, sp.lower_triangle, sp.implicit_unit_diagonal, b, y)
    up = sp.triangular_solve_inspect(lu, sp.upper_triangle, sp.explicit_diagonal, y, x)

    def factor():
        sp.ilu0(info, a, lu)

    def solves():
        sp.triangular_solve(lo, lu, sp.lower_triangle, sp.implicit_unit_diagonal, b, y)
        sp.triangular_solve(up, lu, sp.upper_triangle, sp.explicit_diagonal, y, x)

    for _ in range(3):
        factor()
    status = sp.ilu0_status(info)
    for _ in range(3):
        solves()
    torch.cuda.synchronize()
    tf, ts = [], []
    for _ in range(args.rounds):
        tf.append(round_ms(factor, args.calls))
        ts.append(round_ms(solves, args.calls))
    pi = info.state_.info()
    return {"matrix": name, "dtype": str(dtype).replace("torch.", ""), "m": m, "nnz": nnz, "levels": pi["levels"],
            "max_level_width": pi["max_level_width"], "launches_per_factor": pi["launches_per_factor"],
            "lanes_per_row": pi["lanes_per_row"], "lower_solve_launches": lo.state_.info()["launches_per_solve"],
            "upper_solve_launches": up.state_.info()["launches_per_solve"], "status": status, "factor_ms": stats(tf),
            "solve_pair_ms": stats(ts), "factor_over_solve_pair": round(float(np.median(tf)) / float(np.median(ts)), 3),
            "factor_us_per_level": round(1e3 * float(np.median(tf)) / max(pi["levels"], 1), 3),
            "x_finite": bool(torch.isfinite(x).all())}


def kernel_resources(path):
    """[(kernel, VGPRs, SGPRs, LDS bytes per block, occupancy)] from the compiler's kernel-resource-usage remarks."""
    if not path or not os.path.exists(path):
        return []
    text = open(path).read()
    out = []
    for blk in re.split(r"remark: Function Name: ", text)[1:]:
        name = blk.split()[0]
        if "ilu0" not in name:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
        out.append({"kernel": name, "vgprs": get(r"VGPRs"), "sgprs": get(r"TotalSGPRs"), "lds_bytes": get(r"LDS Size \[bytes/block\]"),
                    "scratch_bytes": get(r"ScratchSize \[bytes/lane\]"), "waves_per_simd": get(r"Occupancy \[waves/SIMD\]")})
    return out


def markdown(out):
    lines = ["# ILU(0): one factor call against the two triangular solves it feeds", "",
             f"Device: {out['device']}.  {out['rounds']} rounds alternating (a) one factor and (b) one lower-unit + one upper-explicit "
             f"vector solve on its result, {out['calls']} calls per round between two device events; ms per call, median (min .. max) "
             "over the rounds.  Written by tools/bench_ilu0.py.", "",
             "| matrix | type | rows | entries | levels | widest | level launches per factor | lanes per row | (a) factor, ms | "
             "(b) solve pair, ms | (a) / (b) | factor us per level | pivots |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        f, s = r["factor_ms"], r["solve_pair_ms"]
        lines.append(f"| {r['matrix']} | {r['dtype']} | {r['m']} | {r['nnz']} | {r['levels']} | {r['max_level_width']} | "
                     f"{r['launches_per_factor']} | {r['lanes_per_row']} | {f['median']} ({f['min']} .. {f['max']}) | "
                     f"{s['median']} ({s['min']} .. {s['max']}) | {r['factor_over_solve_pair']} | {r['factor_us_per_level']} | "
                     f"{'all fine' if r['status'] == -1 else 'first bad row ' + str(r['status'])} |")
    lines += ["", "The solves run as one cooperative launch each outside a graph (launches per solve: "
              + ", ".join(sorted({f"{r['lower_solve_launches']} / {r['upper_solve_launches']}" for r in out["records"]}))
              + " lower / upper); the factor has no cooperative form: one launch per wide level, one per run of narrow levels.", ""]
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--dtypes", nargs="*", default=["float32", "float64"])
    ap.add_argument("--matrices", nargs="*", default=["laplace7", "random9"])
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ilu0.py measures on the GPU: no device, no number"
    dev = torch.device("cuda:0")
    recs = []
    for name in args.matrices:
        for dn in args.dtypes:
            dtype = getattr(torch, dn)
            a = laplace7(args.grid, dtype, dev) if name == "laplace7" else random9(args.rows, dtype, dev)
            recs.append(case(name, a, args, dev))
            print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
            del a
            torch.cuda.empty_cache()
    out = {"metric": "ilu0_factor_vs_solve_pair", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "calls": args.calls, "records": recs, "kernel_resources": kernel_resources(args.resources)}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "ilu0_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(args.out_dir, "ilu0_bench.md"), "w") as f:
        f.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
