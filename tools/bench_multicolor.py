"""The multicolour ordering against the natural one: what multicolor_order and permute cost, and what ilu0 and the exact solve pair
gain or lose on B = P A P^T (csrc/multicolor.hip), fp32 and fp64, on the two matrices of bench_ilu0.py (laplace7, random9: same
generators).  Then the price: preconditioned CG with ILU(0) in both orders on a smaller Laplacian.

Protocol per matrix: multicolor_order and permute_inspect --calls times each, wall clock around the call (both synchronise);
every other inspect once; three warm-up calls; then --rounds rounds that visit, --calls calls each between two device events,
  the value gather permute(info, A, perm, B) and a device-to-device copy of the nnz values,
  ilu0 on A and on B (out of place), the lower-unit + upper-explicit solve pair on A's factor and on B's.
Reported: median (min .. max) over the rounds, levels before and after, colours and rounds, the ratios B / A.
Convergence (--pcg-grid, fp64): CG on the 7-point Laplacian with M = ILU(0), host-driven (one dot product read back per
iteration), to a relative residual of 1e-8, in natural order and on the multicolour-ordered system P A P^T (P x) = P b:
iterations, total time, time per iteration.
Writes multicolor_bench.json and multicolor_bench.md into --out-dir and prints the JSON line."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import spblas_reference_amd as sp  # noqa: E402
from bench_ilu0 import laplace7, random9, round_ms, stats  # noqa: E402

LO = (sp.lower_triangle, sp.implicit_unit_diagonal)
UP = (sp.upper_triangle, sp.explicit_diagonal)


def wall_ms(fn, calls):
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return ts, r


def empty_like_matrix(a):
    m, nnz = a.shape()[0], a.size()
    return sp.csr_view(torch.empty_like(a.values()), torch.empty_like(a.rowptr()), torch.empty_like(a.colind()), (m, m), nnz)


class Precond:
    """ilu0 + the two solves on one matrix, everything inspected once."""

    def __init__(self, a):
        m, nnz = a.shape()[0], a.size()
        self.a = a
        self.lu = sp.csr_view(torch.empty_like(a.values()), a.rowptr(), a.colind(), (m, m), nnz)
        self.y = torch.empty(m, dtype=a.values().dtype, device=a.values().device)
        self.info = sp.ilu0_inspect(a)
        z = torch.empty_like(self.y)
        self.lo = sp.triangular_solve_inspect(self.lu, *LO, z, self.y)
        self.up = sp.triangular_solve_inspect(self.lu, *UP, self.y, z)

    def factor(self):
        sp.ilu0(self.info, self.a, self.lu)

    def apply(self, r, z):
        sp.triangular_solve(self.lo, self.lu, *LO, r, self.y)
        sp.triangular_solve(self.up, self.lu, *UP, self.y, z)

    def levels(self):
        return {"ilu0": self.info.state_.info()["levels"], "lower": self.lo.state_.info()["levels"],
                "upper": self.up.state_.info()["levels"]}


def case(name, a, args, dev):
    dtype = a.values().dtype
    m, nnz = a.shape()[0], a.size()
    t_order, order = wall_ms(lambda: sp.multicolor_order(a), args.calls)
    b = empty_like_matrix(a)
    t_insp, pinfo = wall_ms(lambda: sp.permute_inspect(a, order.perm, b), args.calls)
    sp.permute(pinfo, a, order.perm, b)
    copy_dst = torch.empty_like(a.values())
    pa, pb = Precond(a), Precond(b)
    rhs = torch.rand(m, dtype=dtype, device=dev)
    z = torch.empty_like(rhs)
    variants = {
        "gather": lambda: sp.permute(pinfo, a, order.perm, b),
        "copy": lambda: copy_dst.copy_(a.values()),
        "ilu0_A": pa.factor, "ilu0_B": pb.factor,
        "solves_A": lambda: pa.apply(rhs, z), "solves_B": lambda: pb.apply(rhs, z),
    }
    for fn in variants.values():
        for _ in range(3):
            fn()
    status = (sp.ilu0_status(pa.info), sp.ilu0_status(pb.info))
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            ts[k].append(round_ms(fn, args.calls))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    oi = order.info()
    return {"matrix": name, "dtype": str(dtype).replace("torch.", ""), "m": m, "nnz": nnz, "colors": oi["colors"],
            "rounds": oi["rounds"], "max_color_size": oi["max_color_size"], "lanes_per_row": oi["lanes_per_row"],
            "multicolor_order_ms": stats(t_order), "permute_inspect_ms": stats(t_insp),
            "levels_A": pa.levels(), "levels_B": pb.levels(), "status": status,
            **{k + "_ms": stats(v) for k, v in ts.items()},
            "gather_over_copy": round(med["gather"] / med["copy"], 3),
            "ilu0_B_over_A": round(med["ilu0_B"] / med["ilu0_A"], 3),
            "solves_B_over_A": round(med["solves_B"] / med["solves_A"], 3)}


def pcg(a, pre, rhs, tol, max_iter):
    """Host-driven preconditioned CG; returns (iterations, relative residual, ms)."""
    x = torch.zeros_like(rhs)
    r = rhs.clone()
    z, q = torch.empty_like(rhs), torch.empty_like(rhs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pre.factor()
    pre.apply(r, z)
    p = z.clone()
    rz = torch.dot(r, z)
    norm_b = float(torch.linalg.vector_norm(rhs))
    it, rel = 0, 1.0
    while it < max_iter:
        sp.multiply(a, p, q)
        alpha = rz / torch.dot(p, q)
        x.add_(p, alpha=float(alpha))
        r.sub_(q, alpha=float(alpha))
        it += 1
        rel = float(torch.linalg.vector_norm(r)) / norm_b
        if rel <= tol:
            break
        pre.apply(r, z)
        rz_new = torch.dot(r, z)
        p.mul_(float(rz_new / rz)).add_(z)
        rz = rz_new
    torch.cuda.synchronize()
    return it, rel, 1e3 * (time.perf_counter() - t0), x


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
    xs = {}
    for name, mat, r in (("natural", a, rhs), ("multicolor", b, prhs)):
        pre = Precond(mat)
        pcg(mat, pre, r, args.pcg_tol, 3)                       # warm-up
        runs = [pcg(mat, pre, r, args.pcg_tol, args.pcg_max_iter) for _ in range(3)]
        it, rel, _, xs[name] = runs[0]
        ms = float(np.median([t for _, _, t, _ in runs]))
        out[name] = {"iterations": it, "relative_residual": rel, "total_ms": round(ms, 3), "ms_per_iteration": round(ms / it, 4),
                     "levels": pre.levels()}
    back = torch.empty_like(rhs)
    sp.permute_vector(order.perm, xs["multicolor"], back, inverse=True)
    out["solutions_differ_rel"] = float(torch.linalg.vector_norm(back - xs["natural"]) / torch.linalg.vector_norm(xs["natural"]))
    return out


def kernel_resources(path):
    if not path or not os.path.exists(path):
        return []
    out = []
    for blk in re.split(r"remark: Function Name: ", open(path).read())[1:]:
        name = blk.split()[0]
        if "mc_" not in name and "pm_" not in name:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
        out.append({"kernel": name, "vgprs": get(r"VGPRs"), "sgprs": get(r"TotalSGPRs"), "lds_bytes": get(r"LDS Size \[bytes/block\]"),
                    "scratch_bytes": get(r"ScratchSize \[bytes/lane\]"), "waves_per_simd": get(r"Occupancy \[waves/SIMD\]")})
    return out


def fmt(s):
    return f"{s['median']} ({s['min']} .. {s['max']})"


def markdown(out):
    L = ["# Multicolour ordering: its cost, and ilu0 / the solve pair before and after", "",
         f"Device: {out['device']}.  multicolor_order and permute_inspect: wall clock around {out['calls']} calls each (both "
         f"synchronise).  Everything else: {out['rounds']} rounds visiting every variant, {out['calls']} calls per visit between two "
         "device events; ms per call, median (min .. max).  A = natural order, B = P A P^T.  Written by tools/bench_multicolor.py.", "",
         "| matrix | type | rows | entries | colours | rounds | largest class | multicolor_order, ms | permute_inspect, ms | "
         "value gather, ms | copy of nnz values, ms | gather / copy |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        L.append(f"| {r['matrix']} | {r['dtype']} | {r['m']} | {r['nnz']} | {r['colors']} | {r['rounds']} | {r['max_color_size']} | "
                 f"{fmt(r['multicolor_order_ms'])} | {fmt(r['permute_inspect_ms'])} | {fmt(r['gather_ms'])} | {fmt(r['copy_ms'])} | "
                 f"{r['gather_over_copy']} |")
    L += ["", "| matrix | type | levels A (ilu0 / lower / upper) | levels B | ilu0 on A, ms | ilu0 on B, ms | B / A | solve pair on A, ms | "
          "solve pair on B, ms | B / A | pivots A, B |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        la, lb = r["levels_A"], r["levels_B"]
        L.append(f"| {r['matrix']} | {r['dtype']} | {la['ilu0']} / {la['lower']} / {la['upper']} | {lb['ilu0']} / {lb['lower']} / "
                 f"{lb['upper']} | {fmt(r['ilu0_A_ms'])} | {fmt(r['ilu0_B_ms'])} | {r['ilu0_B_over_A']} | {fmt(r['solves_A_ms'])} | "
                 f"{fmt(r['solves_B_ms'])} | {r['solves_B_over_A']} | {r['status'][0]}, {r['status'][1]} (-1 = all fine) |")
    c = out.get("convergence")
    if c:
        L += ["", f"## The convergence trade: CG with M = ILU(0) on the 7-point Laplacian {c['grid']}^3 ({c['m']} rows), fp64, to "
              f"{c['tolerance']:g}", "", "Host-driven loop (two dot products and a norm read back per iteration), factor included, "
              "median of three runs.", "",
              "| order | levels (ilu0 / lower / upper) | iterations | relative residual | total, ms | ms per iteration |",
              "|---|---|---|---|---|---|"]
        for k in ("natural", "multicolor"):
            v = c[k]
            L.append(f"| {k} | {v['levels']['ilu0']} / {v['levels']['lower']} / {v['levels']['upper']} | {v['iterations']} | "
                     f"{v['relative_residual']:.2e} | {v['total_ms']} | {v['ms_per_iteration']} |")
        L += ["", f"{c['colors']} colours; the two solutions differ by {c['solutions_differ_rel']:.1e} relative to the natural one."]
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
    assert torch.cuda.is_available(), "bench_multicolor.py measures on the GPU: no device, no number"
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
    out = {"metric": "multicolor_order_vs_natural", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "calls": args.calls, "records": recs, "convergence": conv, "kernel_resources": kernel_resources(args.resources)}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "multicolor_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(args.out_dir, "multicolor_bench.md"), "w") as f:
        f.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
