"""The smoothed prolongator P = (I - omega D_F^-1 A_F) T (csrc/smooth.hip): what smooth_prolongator_inspect costs, what the
two-launch value refresh smooth_prolongator costs, and what smoothing the prolongator buys CG with a V-cycle -- on the two
matrices of bench_ilu0.py (laplace7, random9: same generators), fp32 and fp64, by the conventions of bench_aggregate.py.

Protocol per matrix: aggregate once; smooth_prolongator_inspect --calls times, wall clock around the call (it synchronises);
three warm-up calls; then --rounds rounds that visit, --calls calls each between two device events,
  smooth_prolongator(info, A, P, omega, theta = 0)            the value refresh under test,
  multiply_fill(A, T)                                         ONE numeric SpGEMM fill on a pre-computed pattern (a generous
                                                              yardstick: it forms A T alone, no strength rule, no D^-1, no I -),
  a device-to-device copy of the refresh's algorithmic bytes  nnz (value + column + one gathered d_j) + (nnz + m) map entries
                                                              + nnz(P) (value + segment offset) + m (two row offsets, d written
                                                              and read).
Reported: median (min .. max) over the rounds; the refresh's algorithmic bytes over its time as a fraction of the copy's rate;
the relative difference from the SpGEMM route (I - omega D^-1 A) * T at theta = 0 (S built with torch, one SpGEMM).
Convergence (--pcg-grids, fp64): CG on the 7-point Laplacian to 1e-8 with the V-cycle of bench_aggregate.py, the plain
(tentative) prolongator with coarsen against the smoothed one (omega on every level, A_c by transpose and two SpGEMMs):
iterations, operator complexity (entries of all levels over entries of A), set-up, total, ms per iteration; the smoothed cycle
also with its calls recorded in one graph per application.
Writes smooth_bench.json and smooth_bench.md into --out-dir and prints the JSON line."""
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
from bench_aggregate import Level, SpgemmRoute, Vcycle, empty_csr, fmt  # noqa: E402
from bench_ilu0 import laplace7, random9, round_ms, stats  # noqa: E402
from bench_multicolor import pcg, wall_ms  # noqa: E402


def smoothed(a, agg, n_agg, omega, theta=0.0):
    """(info, P) through smooth_prolongator_inspect / _structure / smooth_prolongator."""
    info = sp.smooth_prolongator_inspect(a, agg, n_agg)
    p = empty_csr((a.shape()[0], n_agg), info.nnz, a.values().dtype, a.values().device)
    sp.smooth_prolongator_structure(info, p)
    sp.smooth_prolongator(info, a, p, omega, theta)
    return info, p


def jacobi_smoother_matrix(a, omega):
    """S = I - omega D^-1 A on A's pattern (every row stores its diagonal once: both generators do)."""
    m, nnz = a.shape()[0], a.size()
    rows = torch.repeat_interleave(torch.arange(m, device=a.values().device), torch.diff(a.rowptr().long()))
    on = a.colind().long() == rows
    d = torch.zeros(m, dtype=a.values().dtype, device=a.values().device)
    d[rows[on]] = a.values()[on]
    w = torch.tensor(omega, dtype=a.values().dtype, device=d.device)
    v = -(w / d)[rows] * a.values()
    v = torch.where(on, 1 - w + torch.zeros_like(v), v)
    return sp.csr_view(v, a.rowptr(), a.colind(), (m, m), nnz)


def case(name, a, args, dev):
    dtype = a.values().dtype
    m, nnz = a.shape()[0], a.size()
    es = a.values().element_size()
    res = sp.aggregate(a, args.theta)
    n = res.n_agg
    t_insp, info = wall_ms(lambda: sp.smooth_prolongator_inspect(a, res.agg, n), args.calls)
    pn = info.nnz
    p = empty_csr((m, n), pn, dtype, dev)
    sp.smooth_prolongator_structure(info, p)
    tent = res.prolongator(dtype)
    at, st = SpgemmRoute._symbolic(a, tent, (m, n), dtype, dev)
    alg_bytes = nnz * (es + 4 + es) + (nnz + m) * 4 + pn * (es + 4) + m * (8 + 2 * es)
    src = torch.empty(alg_bytes // 2, dtype=torch.uint8, device=dev)         # a copy reads and writes: half the bytes each way
    dst = torch.empty_like(src)
    variants = {"smooth": lambda: sp.smooth_prolongator(info, a, p, args.omega, 0.0),
                "fill_A_T": lambda: sp.multiply_fill(st, a, tent, at), "copy": lambda: dst.copy_(src)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # against the SpGEMM route (I - omega D^-1 A) * T at theta = 0 (the same terms in another order and association)
    r, _ = SpgemmRoute._symbolic(jacobi_smoother_matrix(a, args.omega), tent, (m, n), dtype, dev)
    same = r.size() == pn and bool(torch.equal(r.colind()[:pn], p.colind()[:pn]))
    diff = float((r.values()[:pn] - p.values()[:pn]).abs().max() / p.values()[:pn].abs().max()) if same else None
    del r
    ts = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            ts[k].append(round_ms(fn, args.calls))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    return {"matrix": name, "dtype": str(dtype).replace("torch.", ""), "m": m, "nnz": nnz, "theta": args.theta,
            "omega": args.omega, "aggregates": n, "p_nnz": pn, "entries_per_row_of_P": round(pn / m, 3),
            "lanes_per_row": res.info()["lanes_per_row"], "inspect_ms": stats(t_insp),
            **{k + "_ms": stats(v) for k, v in ts.items()},
            "refresh_algorithmic_bytes": alg_bytes, "refresh_GBps": round(alg_bytes / med["smooth"] / 1e6, 1),
            "copy_GBps": round(alg_bytes / med["copy"] / 1e6, 1),
            "refresh_fraction_of_copy_rate": round(med["copy"] / med["smooth"], 3),
            "smooth_over_fill": round(med["smooth"] / med["fill_A_T"], 3), "same_pattern_as_spgemm_route": same,
            "differs_from_spgemm_route_rel": diff}


class SmoothLevel(Level):
    """A level of bench_aggregate.py whose coarsen() uses the smoothed prolongator and the SpGEMM route for A_c."""
    omega = 2.0 / 3.0

    def coarsen(self):
        dtype, dev = self.a.values().dtype, self.a.values().device
        self.agg = sp.aggregate(self.a, self.theta)
        n = self.agg.n_agg
        self.info, self.p = smoothed(self.a, self.agg.agg, n, self.omega)
        self.pt = empty_csr((n, self.m), self.p.size(), dtype, dev)
        sp.transpose(self.p, self.pt)
        ap, _ = SpgemmRoute._symbolic(self.a, self.p, (self.m, n), dtype, dev)
        c, _ = SpgemmRoute._symbolic(self.pt, ap, (n, n), dtype, dev)
        return c


class SmoothVcycle(Vcycle):
    def __init__(self, a, theta, coarsest_rows, coarse_sweeps, omega):
        SmoothLevel.omega = omega
        self.levels = [SmoothLevel(a, theta)]
        while self.levels[-1].m >= coarsest_rows:
            nxt = self.levels[-1].coarsen()
            if nxt.shape()[0] >= self.levels[-1].m:
                self.levels[-1].p = None
                break
            self.levels.append(SmoothLevel(nxt, theta))
        self.coarse_sweeps = coarse_sweeps


class Graphed:
    """One application of a V-cycle recorded in a graph: apply() copies r in, replays, copies z out."""

    def __init__(self, vc, m, dtype, dev):
        self.vc = vc
        self.r, self.z = torch.zeros(m, dtype=dtype, device=dev), torch.zeros(m, dtype=dtype, device=dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            vc.apply(self.r, self.z)                                # every call once eagerly on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            vc.apply(self.r, self.z)

    def factor(self):
        pass

    def apply(self, r, z):
        self.r.copy_(r)
        self.graph.replay()
        z.copy_(self.z)


def complexity(vc):
    return round(sum(lv.a.size() for lv in vc.levels) / vc.levels[0].a.size(), 4)


def convergence(grid, args, dev):
    a = laplace7(grid, torch.float64, dev)
    m = a.shape()[0]
    rhs = torch.rand(m, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    out = {"grid": grid, "m": m, "tolerance": args.pcg_tol, "theta": args.pcg_theta, "omega": args.omega,
           "coarse_sweeps": args.coarse_sweeps}
    makers = {"plain": lambda: Vcycle(a, args.pcg_theta, 1000, args.coarse_sweeps),
              "smoothed": lambda: SmoothVcycle(a, args.pcg_theta, 1000, args.coarse_sweeps, args.omega)}
    for name, make in makers.items():
        t_setup, vc = [], None
        for _ in range(3):
            ts, vc = wall_ms(make, 1)
            t_setup += ts
        pres = {"": vc}
        if name == "smoothed" and args.graph:
            try:
                pres["_graph"] = Graphed(vc, m, torch.float64, dev)
            except Exception as e:  # noqa: BLE001  (reported, not hidden: the eager figures stand on their own)
                out["smoothed_graph_error"] = f"{type(e).__name__}: {e}"
        for suffix, pre in pres.items():
            pcg(a, pre, rhs, args.pcg_tol, 3)                       # warm-up
            runs = [pcg(a, pre, rhs, args.pcg_tol, args.pcg_max_iter) for _ in range(3)]
            it, rel = runs[0][0], runs[0][1]
            ms = float(np.median([t for _, _, t, _ in runs]))
            out[name + suffix] = {"iterations": it, "relative_residual": rel, "total_ms": round(ms, 3),
                                  "ms_per_iteration": round(ms / it, 4), "setup_ms": stats(t_setup),
                                  "operator_complexity": complexity(vc),
                                  "levels": [{"rows": lv.m, "nnz": lv.a.size()} for lv in vc.levels]}
    return out


def markdown(out):
    L = ["# The smoothed prolongator: its inspect, the value refresh, a V-cycle in CG", "",
         f"Device: {out['device']}.  smooth_prolongator_inspect: wall clock around {out['calls']} calls (it synchronises).  "
         f"Everything else: {out['rounds']} rounds visiting every variant, {out['calls']} calls per visit between two device "
         "events; ms per call, median (min .. max).  omega = " + f"{out['omega']:.4f}" + ", theta = 0 in the refresh.  "
         "Written by tools/bench_smooth.py.", "",
         "| matrix | type | rows | entries | aggregates | entries of P | per row | lanes | inspect, ms | refresh, ms | "
         "multiply_fill(A, T), ms | refresh / fill | copy of the refresh's bytes, ms | refresh GB/s | copy GB/s | "
         "fraction of the copy rate | differs from (I - w D^-1 A) T (relative) |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        d = r["differs_from_spgemm_route_rel"]
        L.append(f"| {r['matrix']} | {r['dtype']} | {r['m']} | {r['nnz']} | {r['aggregates']} | {r['p_nnz']} | "
                 f"{r['entries_per_row_of_P']} | {r['lanes_per_row']} | {fmt(r['inspect_ms'])} | {fmt(r['smooth_ms'])} | "
                 f"{fmt(r['fill_A_T_ms'])} | {r['smooth_over_fill']} | {fmt(r['copy_ms'])} | {r['refresh_GBps']} | "
                 f"{r['copy_GBps']} | {r['refresh_fraction_of_copy_rate']} | "
                 + (f"{d:.1e}" if d is not None else "other pattern") + " |")
    for c in out.get("convergence") or []:
        L += ["", f"## CG on the 7-point Laplacian {c['grid']}^3 ({c['m']} rows), fp64, to {c['tolerance']:g}", "",
              f"Host-driven loop, median of three runs; the V-cycle of tools/bench_aggregate.py (theta {c['theta']}, a forward sweep "
              f"before and a backward sweep after the correction on every level, {c['coarse_sweeps']} symmetric sweeps on the "
              f"coarsest); smoothed: omega {c['omega']:.4f} on every level, A_c by transpose and two SpGEMMs.", "",
              "| prolongator | iterations | relative residual | operator complexity | levels (rows) | set-up, ms | total, ms | "
              "ms per iteration |", "|---|---|---|---|---|---|---|---|"]
        for k in ("plain", "smoothed", "smoothed_graph"):
            if k in c:
                v = c[k]
                L.append(f"| {k} | {v['iterations']} | {v['relative_residual']:.2e} | {v['operator_complexity']} | "
                         + " -> ".join(str(lv["rows"]) for lv in v["levels"])
                         + f" | {fmt(v['setup_ms'])} | {v['total_ms']} | {v['ms_per_iteration']} |")
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
    ap.add_argument("--theta", type=float, default=0.0)
    ap.add_argument("--omega", type=float, default=2.0 / 3.0)
    ap.add_argument("--pcg-grids", type=int, nargs="*", default=[16, 64])
    ap.add_argument("--pcg-tol", type=float, default=1e-8)
    ap.add_argument("--pcg-theta", type=float, default=0.0)
    ap.add_argument("--pcg-max-iter", type=int, default=2000)
    ap.add_argument("--coarse-sweeps", type=int, default=20)
    ap.add_argument("--graph", type=int, default=1)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_smooth.py measures on the GPU: no device, no number"
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
    conv = []
    for g in args.pcg_grids:
        conv.append(convergence(g, args, dev))
        print(json.dumps(conv[-1]), file=sys.stderr, flush=True)
    out = {"metric": "smooth_prolongator", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "calls": args.calls, "omega": args.omega, "records": recs, "convergence": conv}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "smooth_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(args.out_dir, "smooth_bench.md"), "w") as f:
        f.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
