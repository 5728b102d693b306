"""Multicolour Gauss-Seidel sweeps (csrc/gauss_seidel.hip) against what the preconditioner benches already measure, fp32 and
fp64, on the two matrices of bench_ilu0.py / bench_multicolor.py (laplace7, random9: same generators), coloured by
multicolor_order.

Protocol per matrix: every inspect once; three warm-up calls; then --rounds rounds that visit, --calls calls each between two
device events,
  one forward and one symmetric sweep on A with perm, and on B = P A P^T without one,
  the exact lower-unit + upper-explicit triangular_solve pair on ILU(0) of B (the multicolour preconditioner apply),
  one plan-free multiply(B, x, y).
Reported: median (min .. max) over the rounds, forward-on-B over the solve pair, A-with-perm over B.
What the sweeps buy: the relative residual after 1 .. 5 symmetric sweeps from x = 0 on the Laplacian, and (--pcg-grid, fp64) CG
to a relative residual of 1e-8 with one symmetric sweep from x = 0 as the preconditioner (SSOR), against multicolour ILU(0)
measured in the same run (bench_multicolor.py's loop).
Writes gauss_seidel_bench.json and gauss_seidel_bench.md into --out-dir and prints the JSON line."""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import spblas_reference_amd as sp  # noqa: E402
from bench_ilu0 import laplace7, random9, round_ms, stats  # noqa: E402
from bench_multicolor import Precond, empty_like_matrix, pcg  # noqa: E402


class Sweeper:
    """gauss_seidel on one matrix, inspected once; apply(r, z) is one symmetric sweep from z = 0: the SSOR preconditioner."""

    def __init__(self, a, color_ptr, perm=None):
        self.a = a
        self.info = sp.gauss_seidel_inspect(a, color_ptr, perm)

    def sweep(self, b, x, direction, sweeps=1):
        sp.gauss_seidel(self.info, self.a, b, x, sweeps=sweeps, direction=direction)

    def factor(self):
        pass

    def apply(self, r, z):
        z.zero_()
        sp.gauss_seidel(self.info, self.a, r, z, direction="symmetric")

    def levels(self):
        return self.info.state_.info()


def rel_residual(a, b, x, work):
    sp.multiply(a, x, work)
    return float(torch.linalg.vector_norm(b - work) / torch.linalg.vector_norm(b))


def case(name, a, args, dev):
    dtype = a.values().dtype
    m, nnz = a.shape()[0], a.size()
    order = sp.multicolor_order(a)
    b = empty_like_matrix(a)
    sp.permute(a, order.perm, b)
    on_a, on_b = Sweeper(a, order.color_ptr, order.perm), Sweeper(b, order.color_ptr)
    pre = Precond(b)
    pre.factor()
    rhs = torch.rand(m, dtype=dtype, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    prhs = torch.empty_like(rhs)
    sp.permute_vector(order.perm, rhs, prhs)
    x, px, z, y = (torch.zeros_like(rhs) for _ in range(4))
    variants = {
        "forward_A": lambda: on_a.sweep(rhs, x, "forward"), "symmetric_A": lambda: on_a.sweep(rhs, x, "symmetric"),
        "forward_B": lambda: on_b.sweep(prhs, px, "forward"), "symmetric_B": lambda: on_b.sweep(prhs, px, "symmetric"),
        "solves_B": lambda: pre.apply(prhs, z), "spmv_B": lambda: sp.multiply(b, px, y),
    }
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            ts[k].append(round_ms(fn, args.calls))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    # what the sweeps buy: the relative residual after 1 .. 5 symmetric sweeps from x = 0, and that both forms agree
    px.zero_()
    x.zero_()
    residuals = []
    for _ in range(5):
        on_b.sweep(prhs, px, "symmetric")
        on_a.sweep(rhs, x, "symmetric")
        residuals.append(rel_residual(b, prhs, px, y))
    back = torch.empty_like(rhs)
    sp.permute_vector(order.perm, px, back, inverse=True)
    gi = on_b.levels()
    return {"matrix": name, "dtype": str(dtype).replace("torch.", ""), "m": m, "nnz": nnz, "colors": gi["colors"],
            "max_color_size": gi["max_color_size"], "lanes_per_row": gi["lanes_per_row"],
            "launches_per_forward_sweep": gi["launches_per_forward_sweep"], "levels_B": pre.levels(),
            **{k + "_ms": stats(v) for k, v in ts.items()},
            "forward_B_over_solves_B": round(med["forward_B"] / med["solves_B"], 3),
            "symmetric_B_over_solves_B": round(med["symmetric_B"] / med["solves_B"], 3),
            "forward_A_over_B": round(med["forward_A"] / med["forward_B"], 3),
            "symmetric_A_over_B": round(med["symmetric_A"] / med["symmetric_B"], 3),
            "forward_B_over_spmv_B": round(med["forward_B"] / med["spmv_B"], 3),
            "residual_after_symmetric_sweeps": residuals,
            "A_against_B_rel": float(torch.linalg.vector_norm(back - x) / torch.linalg.vector_norm(x))}


def convergence(args, dev):
    a = laplace7(args.pcg_grid, torch.float64, dev)
    m = a.shape()[0]
    rhs = torch.rand(m, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    order = sp.multicolor_order(a)
    b = empty_like_matrix(a)
    sp.permute(a, order.perm, b)
    prhs = torch.empty_like(rhs)
    sp.permute_vector(order.perm, rhs, prhs)
    out = {"grid": args.pcg_grid, "m": m, "tolerance": args.pcg_tol, "colors": order.info()["colors"]}
    for name, pre in (("ilu0_multicolor", Precond(b)), ("ssor_multicolor", Sweeper(b, order.color_ptr))):
        pcg(b, pre, prhs, args.pcg_tol, 3)                       # warm-up
        runs = [pcg(b, pre, prhs, args.pcg_tol, args.pcg_max_iter) for _ in range(3)]
        it, rel = runs[0][0], runs[0][1]
        ms = float(np.median([t for _, _, t, _ in runs]))
        out[name] = {"iterations": it, "relative_residual": rel, "total_ms": round(ms, 3), "ms_per_iteration": round(ms / it, 4)}
    return out


def kernel_resources(path):
    if not path or not os.path.exists(path):
        return []
    out = []
    for blk in re.split(r"remark: Function Name: ", open(path).read())[1:]:
        name = blk.split()[0]
        if "gs_" not in name:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
        out.append({"kernel": name, "vgprs": get(r"VGPRs"), "sgprs": get(r"TotalSGPRs"), "lds_bytes": get(r"LDS Size \[bytes/block\]"),
                    "scratch_bytes": get(r"ScratchSize \[bytes/lane\]"), "waves_per_simd": get(r"Occupancy \[waves/SIMD\]")})
    return out


def fmt(s):
    return f"{s['median']} ({s['min']} .. {s['max']})"


def markdown(out):
    L = ["# Multicolour Gauss-Seidel sweeps against the exact solve pair and one SpMV", "",
         f"Device: {out['device']}.  {out['rounds']} rounds visiting every variant, {out['calls']} calls per visit between two device "
         "events; ms per call, median (min .. max).  A = natural order, swept with perm; B = P A P^T, swept without.  "
         "Solve pair: the lower-unit + upper-explicit triangular_solve on ILU(0) of B.  Written by tools/bench_gauss_seidel.py.", "",
         "| matrix | type | rows | entries | colours | launches per forward sweep | lanes | forward on B, ms | symmetric on B, ms | "
         "solve pair on B, ms | multiply(B, x, y), ms | forward / pair | symmetric / pair | forward / SpMV |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        L.append(f"| {r['matrix']} | {r['dtype']} | {r['m']} | {r['nnz']} | {r['colors']} | {r['launches_per_forward_sweep']} | "
                 f"{r['lanes_per_row']} | {fmt(r['forward_B_ms'])} | {fmt(r['symmetric_B_ms'])} | {fmt(r['solves_B_ms'])} | "
                 f"{fmt(r['spmv_B_ms'])} | {r['forward_B_over_solves_B']} | {r['symmetric_B_over_solves_B']} | "
                 f"{r['forward_B_over_spmv_B']} |")
    L += ["", "| matrix | type | forward on A with perm, ms | symmetric on A with perm, ms | forward A / B | symmetric A / B | "
          "A against B after 5 sweeps, relative |", "|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        L.append(f"| {r['matrix']} | {r['dtype']} | {fmt(r['forward_A_ms'])} | {fmt(r['symmetric_A_ms'])} | {r['forward_A_over_B']} | "
                 f"{r['symmetric_A_over_B']} | {r['A_against_B_rel']:.1e} |")
    L += ["", "Relative residual || b - A x || / || b || after 1 .. 5 symmetric sweeps from x = 0:", "",
          "| matrix | type | 1 | 2 | 3 | 4 | 5 |", "|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        L.append(f"| {r['matrix']} | {r['dtype']} | " + " | ".join(f"{v:.3e}" for v in r["residual_after_symmetric_sweeps"]) + " |")
    c = out.get("convergence")
    if c:
        L += ["", f"## CG on the 7-point Laplacian {c['grid']}^3 ({c['m']} rows, multicolour order), fp64, to {c['tolerance']:g}", "",
              "Host-driven loop (two dot products and a norm read back per iteration), the factorisation included where there is "
              "one, median of three runs, both rows measured in this run.", "",
              "| preconditioner | iterations | relative residual | total, ms | ms per iteration |", "|---|---|---|---|---|"]
        for k, label in (("ilu0_multicolor", "ILU(0) of B, exact solve pair"), ("ssor_multicolor", "one symmetric sweep from 0")):
            v = c[k]
            L.append(f"| {label} | {v['iterations']} | {v['relative_residual']:.2e} | {v['total_ms']} | {v['ms_per_iteration']} |")
    if out["kernel_resources"]:
        L += ["", "Kernel resources (`-Rpass-analysis=kernel-resource-usage`, gfx950):", "",
              "| kernel | VGPRs | SGPRs | LDS bytes per block | scratch bytes per lane | waves per SIMD |", "|---|---|---|---|---|---|"]
        L += [f"| `{k['kernel']}` | {k['vgprs']} | {k['sgprs']} | {k['lds_bytes']} | {k['scratch_bytes']} | {k['waves_per_simd']} |"
              for k in out["kernel_resources"]]
    L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=160)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--dtypes", nargs="*", default=["float32", "float64"])
    ap.add_argument("--matrices", nargs="*", default=["laplace7", "random9"])
    ap.add_argument("--pcg-grid", type=int, default=64)
    ap.add_argument("--pcg-tol", type=float, default=1e-8)
    ap.add_argument("--pcg-max-iter", type=int, default=2000)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gauss_seidel.py measures on the GPU: no device, no number"
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
    conv = convergence(args, dev) if args.pcg_grid > 0 else None
    out = {"metric": "gauss_seidel_sweeps", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "calls": args.calls, "records": recs, "convergence": conv, "kernel_resources": kernel_resources(args.resources)}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "gauss_seidel_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(args.out_dir, "gauss_seidel_bench.md"), "w") as f:
        f.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
