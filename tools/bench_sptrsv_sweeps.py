"""triangular_solve_sweeps (csrc/sptrsv_sweeps.hip) as an ILU(0) preconditioner apply, against the exact solve pair
(csrc/sptrsv.hip), fp32 and fp64, on the two matrices of tools/bench_ilu0.py (laplace7 on a --grid^3 cube, random9 with --rows
rows).

Protocol per matrix and type: ilu0 once; triangular_solve_inspect for L (lower, unit) and U (upper, explicit); three warm-up
calls of everything; then --rounds rounds that visit, in turn, the exact pair and, for s in --sweeps, the L apply and the U apply
by s sweeps, plan-free and with the plan -- every visit --calls calls between two device events (one synchronisation per visit);
a visit's figure is its time / calls, a case's figure the median over the rounds (min .. max are kept in the JSON).
Relative residual |b - L U x| / |b| of the exact pair and of the sweeps pair (L by s sweeps, then U by s sweeps), computed on the
device with this library's SpMV on the two triangles of the factor.
Bytes of one plan-free sweep, from the shapes: row offsets 4 (m + 1) + columns 4 nnz + values e nnz (a sweep reads whole rows
and masks the other triangle) + b, the previous iterate and the new one 3 e m, e = bytes per value.  The time of ONE sweep is the
slope (t(s_max) - t(s_min)) / (s_max - s_min) of the plan-free L and U applies; its bytes over that time stand next to the rate
of a device-to-device copy of 1 GiB measured in the same run (read + write bytes over time).
Writes sptrsv_sweeps_bench.json and sptrsv_sweeps_bench.md into --out-dir and prints the JSON line."""
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
from bench_ilu0 import laplace7, random9, round_ms, stats  # noqa: E402

LO = (sp.lower_triangle, sp.implicit_unit_diagonal)
UP = (sp.upper_triangle, sp.explicit_diagonal)


def copy_rate_gbs(dev):
    n = 1 << 28  # 1 GiB of float32
    src, dst = torch.empty(n, device=dev), torch.empty(n, device=dev)
    for _ in range(3):
        dst.copy_(src)
    ts = [round_ms(lambda: dst.copy_(src), 5) for _ in range(5)]
    return 2 * 4 * n / (float(np.median(ts)) * 1e-3) / 1e9


def case(name, a, args, dev):
    dtype = a.values().dtype
    e = a.values().element_size()
    m, nnz = a.shape()[0], a.size()
    lu = sp.csr_view(torch.empty_like(a.values()), a.rowptr(), a.colind(), (m, m), nnz)
    sp.ilu0(a, lu)
    b = torch.rand(m, dtype=dtype, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    y, x = torch.empty_like(b), torch.empty_like(b)
    lo = sp.triangular_solve_inspect(lu, *LO, b, y)
    up = sp.triangular_solve_inspect(lu, *UP, y, x)
    # the two triangles of the factor as SpMV operands (the other triangle zeroed), for the residual
    rows = torch.repeat_interleave(torch.arange(m, device=dev), (a.rowptr()[1:] - a.rowptr()[:-1]).long())
    upper = a.colind().long() >= rows
    zero = torch.zeros_like(lu.values())
    u_mat = sp.csr_view(torch.where(upper, lu.values(), zero), a.rowptr(), a.colind(), (m, m), nnz)
    l_mat = sp.csr_view(torch.where(upper, zero, lu.values()), a.rowptr(), a.colind(), (m, m), nnz)
    del rows, upper, zero

    def residual(xv):
        ux, lux = torch.zeros_like(xv), torch.zeros_like(xv)
        sp.multiply(u_mat, xv, ux)
        sp.multiply(l_mat, ux, lux)      # strict part of L; its unit diagonal adds ux
        return float(torch.linalg.vector_norm((b - lux - ux).double()) / torch.linalg.vector_norm(b.double()))

    def exact():
        sp.triangular_solve(lo, lu, *LO, b, y)
        sp.triangular_solve(up, lu, *UP, y, x)

    def apply(tri, info, rhs, out, s):
        if info is None:
            return lambda: sp.triangular_solve_sweeps(lu, *tri, rhs, out, s)
        return lambda: sp.triangular_solve_sweeps(info, lu, *tri, rhs, out, s)

    visits = {"exact_pair": exact}
    for s in args.sweeps:
        for tag, li, ui in (("free", None, None), ("plan", lo, up)):
            visits[f"L_s{s}_{tag}"] = apply(LO, li, b, y, s)
            visits[f"U_s{s}_{tag}"] = apply(UP, ui, y, x, s)
    for fn in visits.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in visits}
    for _ in range(args.rounds):
        for k, fn in visits.items():
            times[k].append(round_ms(fn, args.calls))
    rec = {"matrix": name, "dtype": str(dtype).replace("torch.", ""), "m": m, "nnz": nnz,
           "levels_lower": lo.state_.info()["levels"], "levels_upper": up.state_.info()["levels"],
           "lanes_per_row": lo.state_.info()["lanes_per_row"], "ms": {k: stats(v) for k, v in times.items()}}
    exact()
    rec["residual"] = {"exact_pair": residual(x)}
    for s in args.sweeps:
        apply(LO, None, b, y, s)()
        apply(UP, None, y, x, s)()
        rec["residual"][f"s{s}"] = residual(x)
    med = lambda k: rec["ms"][k]["median"]
    s0, s1 = min(args.sweeps), max(args.sweeps)
    bytes_sweep = 4 * (m + 1) + 4 * nnz + e * nnz + 3 * e * m
    rec["bytes_per_sweep"] = bytes_sweep
    for tri in ("L", "U"):
        per = (med(f"{tri}_s{s1}_free") - med(f"{tri}_s{s0}_free")) / (s1 - s0) if s1 > s0 else med(f"{tri}_s{s0}_free") / (s0 + 1)
        rec[f"{tri}_ms_per_sweep"] = round(per, 4)
        rec[f"{tri}_gbs"] = round(bytes_sweep / (per * 1e-3) / 1e9, 1) if per > 0 else None
    return rec


def markdown(out):
    sw = out["sweeps"]
    lines = ["# triangular_solve_sweeps: an ILU(0) apply by Jacobi sweeps against the exact solve pair", "",
             f"Device: {out['device']}.  {out['rounds']} rounds, {out['calls']} calls per visit between two device events; ms per "
             "call, median over the rounds.  L = lower / unit, U = upper / explicit on the one ILU(0) factor.  A call with s sweeps "
             "is s + 1 launches.  Residual = |b - L U x| / |b| after the L apply and the U apply with the same s.  Written by "
             "tools/bench_sptrsv_sweeps.py.", "",
             "| matrix | type | rows | entries | levels L / U | lanes | exact pair, ms | exact residual | "
             + " | ".join(f"s={s}: L + U plan-free, ms | s={s}: L + U with plan, ms | s={s} residual" for s in sw) + " |",
             "|---|---|---|---|---|---|---|---|" + "---|---|---|" * len(sw)]
    for r in out["records"]:
        med = lambda k: r["ms"][k]["median"]
        cells = []
        for s in sw:
            cells += [f"{med(f'L_s{s}_free')} + {med(f'U_s{s}_free')} = {med(f'L_s{s}_free') + med(f'U_s{s}_free'):.4f}",
                      f"{med(f'L_s{s}_plan')} + {med(f'U_s{s}_plan')} = {med(f'L_s{s}_plan') + med(f'U_s{s}_plan'):.4f}",
                      f"{r['residual'][f's{s}']:.3e}"]
        lines.append(f"| {r['matrix']} | {r['dtype']} | {r['m']} | {r['nnz']} | {r['levels_lower']} / {r['levels_upper']} | "
                     f"{r['lanes_per_row']} | {med('exact_pair')} | {r['residual']['exact_pair']:.3e} | " + " | ".join(cells) + " |")
    lines += ["", f"One plan-free sweep (slope between s = {min(sw)} and s = {max(sw)}) against the copy rate of this run, "
              f"{out['copy_gbs']:.0f} GB/s (device-to-device copy of 1 GiB, read + write bytes):", "",
              "| matrix | type | bytes per sweep | L: ms per sweep | L: GB/s | L: share of the copy rate | U: ms per sweep | U: GB/s | "
              "U: share of the copy rate |", "|---|---|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        share = lambda g: f"{100 * g / out['copy_gbs']:.0f} %" if g else "-"
        lines.append(f"| {r['matrix']} | {r['dtype']} | {r['bytes_per_sweep']} | {r['L_ms_per_sweep']} | {r['L_gbs']} | "
                     f"{share(r['L_gbs'])} | {r['U_ms_per_sweep']} | {r['U_gbs']} | {share(r['U_gbs'])} |")
    lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=160)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sweeps", type=int, nargs="*", default=[1, 2, 3, 5])
    ap.add_argument("--dtypes", nargs="*", default=["float32", "float64"])
    ap.add_argument("--matrices", nargs="*", default=["laplace7", "random9"])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sptrsv_sweeps.py measures on the GPU: no device, no number"
    dev = torch.device("cuda:0")
    copy_gbs = copy_rate_gbs(dev)
    recs = []
    for name in args.matrices:
        for dn in args.dtypes:
            dtype = getattr(torch, dn)
            a = laplace7(args.grid, dtype, dev) if name == "laplace7" else random9(args.rows, dtype, dev)
            recs.append(case(name, a, args, dev))
            print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
            del a
            torch.cuda.empty_cache()
    out = {"metric": "sptrsv_sweeps_vs_exact_pair", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "calls": args.calls, "sweeps": args.sweeps, "copy_gbs": round(copy_gbs, 1), "records": recs}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "sptrsv_sweeps_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(args.out_dir, "sptrsv_sweeps_bench.md"), "w") as f:
        f.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
