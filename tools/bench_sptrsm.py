"""Triangular solve with a block of right-hand sides against a loop of vector solves (csrc/sptrsm.hip vs csrc/sptrsv.hip).

Matrix: the 4 M-row lower-triangular system bench.py --full and tests/test_gpu_sptrsv.py use (8 random strict entries per
row + the diagonal stored last, 36 M entries, 246 levels).  Cases: fp32 / fp64 x n in {1, 2, 4, 8, 16, 32, 64} x both dense
operands layout_right ("RR") or both layout_left ("LL").  Two timings per case, with ONE plan:
  (a) loop    n vector solves, column by column, on CONTIGUOUS columns (for "RR" a column-major copy of the same data: a
              strided column cannot be passed to the vector solve, and the copy a user would have to make is not timed);
  (b) block   one matrix solve.
Protocol: three warm-up calls of each, then --rounds rounds alternating (a) and (b) in this process, every round --calls
calls between two device events (one synchronisation per round); a round's figure is its time / calls.  Reported per case:
median, min and max over the rounds of both, ms per right-hand side of the block solve, and the block solve's share of the HBM
roofline over ALGORITHMIC bytes nnz (4 + sizeof T) + 2 m n sizeof T at 8 TB/s (an end-to-end figure of a latency-bound
solve, not a kernel's share of peak).  "block_wins" is the acceptance comparison: the slowest round of (b) is faster than the
fastest round of (a).
Writes sptrsm_bench.json and sptrsm_bench.md into --out-dir and prints the JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import spblas_reference_amd as sp  # noqa: E402

HBM = 8.0e12
NS = (1, 2, 4, 8, 16, 32, 64)


def bench_matrix(m, k, dtype, dev):
    """tests/test_gpu_sptrsv.py::test_lower_solve_at_bench_size_every_row: same construction, same seed."""
    g = torch.Generator(device=dev).manual_seed(0)
    rows = torch.arange(m, device=dev).repeat_interleave(k)
    cols = (torch.rand(m * k, device=dev, generator=g, dtype=torch.float64) * rows.double()).long().clamp_(min=0)
    cols = torch.minimum(cols, rows)
    vals = (torch.rand(m * k, device=dev, generator=g) - 0.5) * (0.5 / k)
    rp = torch.arange(m + 1, device=dev, dtype=torch.int64) * (k + 1)
    colind = torch.empty(m * (k + 1), dtype=torch.int32, device=dev)
    values = torch.empty(m * (k + 1), device=dev)
    colind.view(m, k + 1)[:, :k] = cols.view(m, k).int()
    colind.view(m, k + 1)[:, k] = torch.arange(m, device=dev, dtype=torch.int32)
    values.view(m, k + 1)[:, :k] = vals.view(m, k)
    values.view(m, k + 1)[:, k] = 1.0 + torch.rand(m, device=dev, generator=g)
    return sp.csr_view(values.to(dtype), rp.int(), colind, (m, m), m * (k + 1))


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


def case(a, info, m, nnz, n, dtype, layout, args, dev):
    lo, ex = sp.lower_triangle, sp.explicit_diagonal
    g = torch.Generator(device=dev).manual_seed(100 + n)
    cols_b = torch.rand((n, m), dtype=dtype, device=dev, generator=g)     # row j = right-hand side j, contiguous
    cols_x = torch.empty((n, m), dtype=dtype, device=dev)
    if layout == "LL":
        B, X = cols_b.t(), torch.empty((n, m), dtype=dtype, device=dev).t()
    else:
        B, X = cols_b.t().contiguous(), torch.empty((m, n), dtype=dtype, device=dev)

    def loop():
        for j in range(n):
            sp.triangular_solve(info, a, lo, ex, cols_b[j], cols_x[j])

    def block():
        sp.triangular_solve(info, a, lo, ex, B, X)

    for _ in range(3):
        loop()
    for _ in range(3):
        block()
    torch.cuda.synchronize()
    diff = float((X - cols_x.t()).abs().max() / cols_x.abs().max())   # the two must solve the same systems
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(round_ms(loop, args.calls))
        tb.append(round_ms(block, args.calls))
    s = torch.empty((), dtype=dtype).element_size()
    nbytes = nnz * (4 + s) + 2 * m * n * s
    rec = {"dtype": str(dtype).replace("torch.", ""), "layout": layout, "n": n, "loop_ms": stats(ta), "block_ms": stats(tb),
           "block_ms_per_rhs": round(float(np.median(tb)) / n, 4),
           "speedup_median": round(float(np.median(ta)) / float(np.median(tb)), 3),
           "block_wins": bool(max(tb) < min(ta)), "loop_wins": bool(max(ta) < min(tb)),
           "alg_bytes": nbytes, "block_frac_8TBs_alg_bytes": round(nbytes / (float(np.median(tb)) * 1e-3) / HBM, 4),
           "max_rel_diff_block_vs_loop": diff}
    return rec


def markdown(out):
    lines = ["# Triangular solve: one block solve against n vector solves", "",
             f"Device: {out['device']}.  Matrix: {out['m']} rows, {out['nnz']} entries, {out['levels']} levels, "
             f"{out['lanes_per_row']} lanes per row.  {out['rounds']} rounds alternating (a) and (b), {out['calls']} calls per round "
             "between two device events; ms per call, median (min .. max) over the rounds.  Written by tools/bench_sptrsm.py.",
             "", "| type | layout | n | (a) n vector solves, ms | (b) one block solve, ms | (a) / (b) | ms per rhs (b) | "
             "share of 8 TB/s over algorithmic bytes (b) | verdict |", "|---|---|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        la, lb = r["loop_ms"], r["block_ms"]
        verdict = "block faster beyond the spread" if r["block_wins"] else (
            "loop faster beyond the spread" if r["loop_wins"] else "within the spread")
        lines.append(f"| {r['dtype']} | {r['layout']} | {r['n']} | {la['median']} ({la['min']} .. {la['max']}) | "
                     f"{lb['median']} ({lb['min']} .. {lb['max']}) | {r['speedup_median']} | {r['block_ms_per_rhs']} | "
                     f"{100 * r['block_frac_8TBs_alg_bytes']:.1f} % | {verdict} |")
    lines += ["", f"Acceptance (layout_right, both types, every n >= 4: slowest round of (b) faster than the fastest round of (a)): "
              f"{'met' if out['acceptance_met'] else 'NOT met: ' + ', '.join(out['acceptance_failures'])}.",
              "", f"Cooperative one-launch form of the block solve: {out['cooperative_form']}.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--ns", type=int, nargs="*", default=list(NS))
    ap.add_argument("--dtypes", nargs="*", default=["float32", "float64"])
    ap.add_argument("--layouts", nargs="*", default=["RR", "LL"])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sptrsm.py measures on the GPU: no device, no number"
    dev = torch.device("cuda:0")
    m, k = args.rows, 8
    recs, levels, lanes = [], None, None
    for dn in args.dtypes:
        dtype = getattr(torch, dn)
        a = bench_matrix(m, k, dtype, dev)
        b0, x0 = torch.rand(m, dtype=dtype, device=dev), torch.empty(m, dtype=dtype, device=dev)
        info = sp.triangular_solve_inspect(a, sp.lower_triangle, sp.explicit_diagonal, b0, x0)
        pi = info.state_.info()
        levels, lanes = pi["levels"], pi["lanes_per_row"]
        for layout in args.layouts:
            for n in args.ns:
                recs.append(case(a, info, m, a.size(), n, dtype, layout, args, dev))
                print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
        info.state_.check_status()
        del a, info
        torch.cuda.empty_cache()
    fails = [f"{r['dtype']} n={r['n']}" for r in recs if r["layout"] == "RR" and r["n"] >= 4 and not r["block_wins"]]
    out = {"metric": "sptrsm_block_vs_vector_loop", "device": torch.cuda.get_device_name(0), "m": m, "nnz": m * (k + 1),
           "levels": levels, "lanes_per_row": lanes, "rounds": args.rounds, "calls": args.calls, "records": recs,
           "acceptance_met": not fails, "acceptance_failures": fails,
           "cooperative_form": "not shipped: built once and measured slower than one launch per level group at every n (DESIGN.md section 4)"}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "sptrsm_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(args.out_dir, "sptrsm_bench.md"), "w") as f:
        f.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
