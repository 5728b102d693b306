"""MIS-2 aggregation and the Galerkin coarse matrix (csrc/aggregate.hip): what aggregate and coarsen_inspect cost, what the
one-launch value refresh coarsen costs next to the numeric refresh of the route through the existing operations, and what a
V-cycle built from them buys CG -- on the two matrices of bench_ilu0.py (laplace7, random9: same generators), fp32 and fp64.

Protocol per matrix: aggregate, multicolor_order (the other graph algorithm that runs in rounds, same run) and coarsen_inspect
--calls times each, wall clock around the call (all three synchronise); three warm-up calls; then --rounds rounds that visit,
--calls calls each between two device events,
  coarsen(info, A, A_c)                                       the value refresh under test,
  multiply_fill(A, P) then multiply_fill(P^T, A P)            the numeric refresh of the SpGEMM route on its pre-computed
                                                              patterns (P^T is formed once: P does not change with A's values),
  a device-to-device copy of the refresh's algorithmic bytes  nnz (value + map) + nnz(A_c) (value + segment offset).
Reported: median (min .. max) over the rounds; the refresh's algorithmic bytes over its time as a fraction of the copy's rate.
Convergence (--pcg-grid, fp64): CG on the 7-point Laplacian to 1e-8 with a V-cycle preconditioner -- aggregate / coarsen repeated
until fewer than 1 000 rows, a forward multicolour Gauss-Seidel sweep before and a backward one after the correction on every
level (one symmetric sweep around it, so the cycle is symmetric), --coarse-sweeps symmetric sweeps on the coarsest level -- next
to SSOR and multicolour ILU(0) in the same run, host-driven loop as in bench_multicolor.py.
Writes aggregate_bench.json and aggregate_bench.md into --out-dir and prints the JSON line."""
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
from bench_gauss_seidel import Sweeper  # noqa: E402
from bench_ilu0 import laplace7, random9, round_ms, stats  # noqa: E402
from bench_multicolor import Precond, empty_like_matrix, pcg, wall_ms  # noqa: E402


def empty_csr(shape, nnz, dtype, dev):
    return sp.csr_view(torch.empty(nnz, dtype=dtype, device=dev), torch.empty(shape[0] + 1, dtype=torch.int32, device=dev),
                       torch.empty(nnz, dtype=torch.int32, device=dev), shape, nnz)


def galerkin(a, agg, n_agg):
    """(info, A_c) through coarsen_inspect / coarsen_structure / coarsen."""
    info = sp.coarsen_inspect(a, agg, n_agg)
    c = empty_csr((n_agg, n_agg), info.nnz, a.values().dtype, a.values().device)
    sp.coarsen_structure(info, c)
    sp.coarsen(info, a, c)
    return info, c


class SpgemmRoute:
    """A_c = P^T (A P) through transpose and two SpGEMMs: the symbolic passes once, refresh() = the two numeric fills."""

    def __init__(self, a, p):
        dtype, dev = a.values().dtype, a.values().device
        m, n = p.shape()
        self.a, self.p = a, p
        self.pt = empty_csr((n, m), m, dtype, dev)
        sp.transpose(p, self.pt)
        self.ap, self.s1 = self._symbolic(a, p, (m, n), dtype, dev)
        self.c, self.s2 = self._symbolic(self.pt, self.ap, (n, n), dtype, dev)

    @staticmethod
    def _symbolic(x, y, shape, dtype, dev):
        rp = torch.zeros(shape[0] + 1, dtype=torch.int32, device=dev)
        z = sp.csr_view(None, rp, None, shape, 0)
        st = sp.multiply_compute(x, y, z)
        k = st.result_nnz()
        z.update(torch.zeros(k, dtype=dtype, device=dev), rp, torch.zeros(k, dtype=torch.int32, device=dev), shape, k)
        sp.multiply_fill(st, x, y, z)
        return z, st

    def refresh(self):
        sp.multiply_fill(self.s1, self.a, self.p, self.ap)
        sp.multiply_fill(self.s2, self.pt, self.ap, self.c)


def case(name, a, theta, args, dev):
    dtype = a.values().dtype
    m, nnz = a.shape()[0], a.size()
    es = a.values().element_size()
    t_agg, res = wall_ms(lambda: sp.aggregate(a, theta), args.calls)
    t_mc, order = wall_ms(lambda: sp.multicolor_order(a), args.calls)
    t_insp, info = wall_ms(lambda: sp.coarsen_inspect(a, res.agg, res.n_agg), args.calls)
    n, cn = res.n_agg, info.nnz
    c = empty_csr((n, n), cn, dtype, dev)
    sp.coarsen_structure(info, c)
    route = SpgemmRoute(a, res.prolongator(dtype))
    alg_bytes = nnz * (es + 4) + cn * (es + 4)
    src = torch.empty(alg_bytes // 2, dtype=torch.uint8, device=dev)         # a copy reads and writes: half the bytes each way
    dst = torch.empty_like(src)
    variants = {"coarsen": lambda: sp.coarsen(info, a, c), "spgemm_route": route.refresh, "copy": lambda: dst.copy_(src)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the two routes agree (different summation orders: to rounding)
    import scipy.sparse as sps
    host = lambda t: t.cpu().numpy()
    C = sps.csr_matrix((host(c.values()).astype(np.float64), host(c.colind()), host(c.rowptr())), shape=(n, n))
    R = sps.csr_matrix((host(route.c.values()).astype(np.float64), host(route.c.colind()), host(route.c.rowptr())), shape=(n, n))
    diff = float(abs(C - R).max() / abs(C).max())
    ts = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            ts[k].append(round_ms(fn, args.calls))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    ai, oi = res.info(), order.info()
    copy_rate = alg_bytes / med["copy"]
    return {"matrix": name, "dtype": str(dtype).replace("torch.", ""), "m": m, "nnz": nnz, "theta": theta,
            "aggregates": n, "coarse_nnz": cn, "coarsening_ratio": round(m / max(n, 1), 3), "aggregate_rounds": ai["rounds"],
            "largest": ai["largest"], "smallest": ai["smallest"], "singletons": ai["singletons"],
            "strong_entries": ai["strong_entries"], "lanes_per_row": ai["lanes_per_row"],
            "colors": oi["colors"], "multicolor_rounds": oi["rounds"],
            "aggregate_ms": stats(t_agg), "multicolor_order_ms": stats(t_mc), "coarsen_inspect_ms": stats(t_insp),
            **{k + "_ms": stats(v) for k, v in ts.items()},
            "refresh_algorithmic_bytes": alg_bytes, "refresh_GBps": round(alg_bytes / med["coarsen"] / 1e6, 1),
            "copy_GBps": round(copy_rate / 1e6, 1), "refresh_fraction_of_copy_rate": round(med["copy"] / med["coarsen"], 3),
            "coarsen_over_spgemm_route": round(med["coarsen"] / med["spgemm_route"], 3), "routes_differ_rel": diff}


class Level:
    def __init__(self, a, theta):
        dtype, dev = a.values().dtype, a.values().device
        self.a, self.m = a, a.shape()[0]
        self.order = sp.multicolor_order(a)
        self.gs = sp.gauss_seidel_inspect(a, self.order.color_ptr, self.order.perm)
        self.x, self.r, self.w = (torch.zeros(self.m, dtype=dtype, device=dev) for _ in range(3))
        self.p = self.pt = self.agg = None
        self.theta = theta

    def coarsen(self):
        dtype, dev = self.a.values().dtype, self.a.values().device
        self.agg = sp.aggregate(self.a, self.theta)
        n = self.agg.n_agg
        self.p = self.agg.prolongator(dtype)
        self.pt = empty_csr((n, self.m), self.m, dtype, dev)
        sp.transpose(self.p, self.pt)
        self.info, c = galerkin(self.a, self.agg.agg, n)
        return c


class Vcycle:
    """apply(r, z): z = one V-cycle on A z = r from z = 0."""

    def __init__(self, a, theta, coarsest_rows, coarse_sweeps):
        self.levels = [Level(a, theta)]
        while self.levels[-1].m >= coarsest_rows:
            nxt = self.levels[-1].coarsen()
            if nxt.shape()[0] >= self.levels[-1].m:          # nothing strong left: no further level
                self.levels[-1].p = None
                break
            self.levels.append(Level(nxt, theta))
        self.coarse_sweeps = coarse_sweeps

    def factor(self):
        pass

    def cycle(self, k, r, z):
        lv = self.levels[k]
        z.zero_()
        if k == len(self.levels) - 1 or lv.p is None:
            sp.gauss_seidel(lv.gs, lv.a, r, z, sweeps=self.coarse_sweeps, direction="symmetric")
            return
        nxt = self.levels[k + 1]
        sp.gauss_seidel(lv.gs, lv.a, r, z, direction="forward")
        sp.multiply(lv.a, z, lv.w)
        torch.sub(r, lv.w, out=lv.w)
        sp.multiply(lv.pt, lv.w, nxt.r)
        self.cycle(k + 1, nxt.r, nxt.x)
        sp.multiply(lv.p, nxt.x, lv.w)
        z.add_(lv.w)
        sp.gauss_seidel(lv.gs, lv.a, r, z, direction="backward")

    def apply(self, r, z):
        self.cycle(0, r, z)

    def describe(self):
        return [{"rows": lv.m, "nnz": lv.a.size(), "colors": lv.order.info()["colors"],
                 "aggregate_rounds": lv.agg.info()["rounds"] if lv.agg is not None else None} for lv in self.levels]


def convergence(args, dev):
    a = laplace7(args.pcg_grid, torch.float64, dev)
    m = a.shape()[0]
    rhs = torch.rand(m, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    order = sp.multicolor_order(a)
    b = empty_like_matrix(a)
    sp.permute(a, order.perm, b)
    prhs = torch.empty_like(rhs)
    sp.permute_vector(order.perm, rhs, prhs)
    out = {"grid": args.pcg_grid, "m": m, "tolerance": args.pcg_tol, "theta": args.pcg_theta, "coarse_sweeps": args.coarse_sweeps}
    vc, t_setup = None, []
    for _ in range(3):
        ts, vc = wall_ms(lambda: Vcycle(a, args.pcg_theta, 1000, args.coarse_sweeps), 1)
        t_setup += ts
    out["vcycle_setup_ms"] = stats(t_setup)
    out["levels"] = vc.describe()
    for name, mat, r, pre in (("ilu0_multicolor", b, prhs, Precond(b)), ("ssor_multicolor", b, prhs, Sweeper(b, order.color_ptr)),
                              ("vcycle", a, rhs, vc)):
        pcg(mat, pre, r, args.pcg_tol, 3)                       # warm-up
        runs = [pcg(mat, pre, r, args.pcg_tol, args.pcg_max_iter) for _ in range(3)]
        it, rel = runs[0][0], runs[0][1]
        ms = float(np.median([t for _, _, t, _ in runs]))
        out[name] = {"iterations": it, "relative_residual": rel, "total_ms": round(ms, 3), "ms_per_iteration": round(ms / it, 4)}
    return out


def fmt(s):
    return f"{s['median']} ({s['min']} .. {s['max']})"


def markdown(out):
    L = ["# MIS-2 aggregation and the Galerkin coarse matrix: their cost, the value refresh, a V-cycle in CG", "",
         f"Device: {out['device']}.  aggregate, multicolor_order and coarsen_inspect: wall clock around {out['calls']} calls each "
         f"(all synchronise).  Everything else: {out['rounds']} rounds visiting every variant, {out['calls']} calls per visit "
         "between two device events; ms per call, median (min .. max).  Written by tools/bench_aggregate.py.", "",
         "| matrix | type | rows | entries | theta | aggregates | rows per aggregate | smallest .. largest | singletons | rounds | "
         "aggregate, ms | colours | rounds | multicolor_order, ms |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        L.append(f"| {r['matrix']} | {r['dtype']} | {r['m']} | {r['nnz']} | {r['theta']} | {r['aggregates']} | "
                 f"{r['coarsening_ratio']} | {r['smallest']} .. {r['largest']} | {r['singletons']} | {r['aggregate_rounds']} | "
                 f"{fmt(r['aggregate_ms'])} | {r['colors']} | {r['multicolor_rounds']} | {fmt(r['multicolor_order_ms'])} |")
    L += ["", "| matrix | type | entries of A_c | coarsen_inspect, ms | coarsen (refresh), ms | two multiply_fills, ms | "
          "coarsen / fills | copy of the refresh's bytes, ms | refresh GB/s | copy GB/s | fraction of the copy rate | "
          "routes differ (relative) |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["records"]:
        L.append(f"| {r['matrix']} | {r['dtype']} | {r['coarse_nnz']} | {fmt(r['coarsen_inspect_ms'])} | {fmt(r['coarsen_ms'])} | "
                 f"{fmt(r['spgemm_route_ms'])} | {r['coarsen_over_spgemm_route']} | {fmt(r['copy_ms'])} | {r['refresh_GBps']} | "
                 f"{r['copy_GBps']} | {r['refresh_fraction_of_copy_rate']} | {r['routes_differ_rel']:.1e} |")
    c = out.get("convergence")
    if c:
        L += ["", f"## CG on the 7-point Laplacian {c['grid']}^3 ({c['m']} rows), fp64, to {c['tolerance']:g}", "",
              f"Host-driven loop, median of three runs.  V-cycle: theta {c['theta']}, levels "
              + " -> ".join(f"{lv['rows']} rows / {lv['nnz']} entries / {lv['colors']} colours" for lv in c["levels"])
              + f"; a forward sweep before and a backward sweep after the correction on every level, {c['coarse_sweeps']} symmetric "
              f"sweeps on the coarsest; set-up (colourings, aggregations, coarse matrices, transposes) {fmt(c['vcycle_setup_ms'])} ms.",
              "", "| preconditioner | iterations | relative residual | total, ms | ms per iteration |", "|---|---|---|---|---|"]
        for k in ("ilu0_multicolor", "ssor_multicolor", "vcycle"):
            v = c[k]
            L.append(f"| {k} | {v['iterations']} | {v['relative_residual']:.2e} | {v['total_ms']} | {v['ms_per_iteration']} |")
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
    ap.add_argument("--pcg-grid", type=int, default=64)
    ap.add_argument("--pcg-tol", type=float, default=1e-8)
    ap.add_argument("--pcg-theta", type=float, default=0.0)
    ap.add_argument("--pcg-max-iter", type=int, default=2000)
    ap.add_argument("--coarse-sweeps", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_aggregate.py measures on the GPU: no device, no number"
    dev = torch.device("cuda:0")
    recs = []
    for name in args.matrices:
        for dn in args.dtypes:
            dtype = getattr(torch, dn)
            a = laplace7(args.grid, dtype, dev) if name == "laplace7" else random9(args.rows, dtype, dev)
            recs.append(case(name, a, args.theta, args, dev))
            print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
            del a
            torch.cuda.empty_cache()
    conv = convergence(args, dev) if args.pcg_grid > 0 else None
    out = {"metric": "aggregate_and_coarsen", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "calls": args.calls, "records": recs, "convergence": conv}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "aggregate_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(args.out_dir, "aggregate_bench.md"), "w") as f:
        f.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
