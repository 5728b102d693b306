"""Complex SpMV / SpMM measurements (csrc/complex.hip), one JSON line on stdout.

Cases (device-event times, median of --steps after --warmup):
  SpMV at cfg2's shape (10 M x 10 M, 10 entries per row, columns uniform) and on a banded matrix of the same size (10
  entries per row within +-64 columns of the diagonal): c32 / c64, plain and conj(A), plan-free and ROWBLOCK -- next to
  fp64 (c32's bytes) and fp32 through the same plans on the same structure, the yardsticks of the same run.
  SpMM at cfg3's A (2 M x 2 M, 32 entries per row uniform): c64 with n = 64 against fp64 with n = 128 (the same bytes).
Every record: ms, algorithmic bytes (per entry 4 + s, per row sizeof(offset) + s for y plus the offsets, per column s for x;
s = value size), the fraction of 8 TB/s, and the worst error of 4096 sampled rows against complex128 / float64 on the host.
--rocprof: afterwards a second run of this script with --steps 5 under `rocprofv3 --kernel-trace --stats` (its own time
limit); the kernel table of that run is added to the JSON line as "kernel_stats".
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import spblas_reference_amd as sp  # noqa: E402
from spblas_reference_amd import _capi  # noqa: E402

HBM = 8.0e12


def uniform_csr(m, n, per, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    rowptr = torch.arange(0, m * per + 1, per, dtype=torch.int32, device=dev)
    colind = torch.randint(0, n, (m * per,), dtype=torch.int32, device=dev, generator=g)
    return rowptr, colind


def banded_csr(m, per, half, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    rowptr = torch.arange(0, m * per + 1, per, dtype=torch.int32, device=dev)
    rows = torch.arange(m, device=dev, dtype=torch.int64).repeat_interleave(per)
    off = torch.randint(-half, half + 1, (m * per,), device=dev, generator=g)
    colind = (rows + off).clamp_(0, m - 1).to(torch.int32)
    colind = colind.view(m, per).sort(dim=1).values.reshape(-1).contiguous()
    return rowptr, colind


def rand_values(nnz, dtype, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    if dtype.is_complex:
        real = torch.float32 if dtype == torch.complex64 else torch.float64
        return torch.complex(torch.rand(nnz, dtype=real, device=dev, generator=g) - 0.5,
                             torch.rand(nnz, dtype=real, device=dev, generator=g) - 0.5)
    return torch.rand(nnz, dtype=dtype, device=dev, generator=g) - 0.5


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def sample_error(rowptr, colind, values, x, y, conj_a, rows):
    """worst |y - ref| / sum |a||x| over the sampled rows, reference in complex128 / float64 on the host"""
    rp = rowptr.cpu().numpy().astype(np.int64)
    lo, hi = rp[rows], rp[rows + 1]
    idx = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)])
    it = torch.from_numpy(idx).to(values.device)
    v = values[it].cpu().numpy().astype(np.complex128)
    ct = colind[it].long()
    xv = x[ct].cpu().numpy().astype(np.complex128)  # (gathered on the device: only the sampled rows' operands travel)
    if conj_a:
        v = np.conj(v)
    seg = np.repeat(np.arange(len(rows)), hi - lo)
    prod = v[:, None] * xv if xv.ndim == 2 else v * xv
    ref = np.zeros((len(rows),) + prod.shape[1:], dtype=np.complex128)
    np.add.at(ref, seg, prod)
    absr = np.zeros(ref.shape)
    np.add.at(absr, seg, np.abs(v)[:, None] * np.abs(xv) if xv.ndim == 2 else np.abs(v) * np.abs(xv))
    got = y[torch.from_numpy(rows).to(y.device)].cpu().numpy().astype(np.complex128)
    return float(np.max(np.abs(got - ref) / np.maximum(absr, 1e-300)))


def spmv_case(name, rowptr, colind, m, n, dtype, conj_a, plan, args, dev, rng):
    values = rand_values(colind.numel(), dtype, dev, 1)
    x = rand_values(n, dtype, dev, 2)
    y = torch.empty(m, dtype=dtype, device=dev)
    a = sp.csr_view(values, rowptr, colind, (m, n), colind.numel())
    aa = sp.conjugated(a) if conj_a else a
    info = sp.multiply_inspect(aa, x, y, alg=_capi.SPMV_ROWBLOCK) if plan else None
    fn = (lambda: sp.multiply(info, aa, x, y)) if plan else (lambda: sp.multiply(aa, x, y))
    ms = timed(fn, args.steps, args.warmup)
    s = values.element_size()
    nbytes = colind.numel() * (4 + s) + (m + 1) * 4 + n * s + m * s
    rows = np.sort(rng.choice(m, 4096, replace=False))
    err = sample_error(rowptr, colind, values, x, y, conj_a, rows)
    return {"case": name, "dtype": str(dtype).replace("torch.", ""), "conj_a": conj_a, "plan": "rowblock" if plan else "plan_free",
            "ms": round(ms, 4), "alg_bytes": nbytes, "frac_8TBs": round(nbytes / (ms * 1e-3) / HBM, 3),
            "max_rel_err_sampled": err}


def spmm_case(name, rowptr, colind, m, k, n, dtype, args, dev, rng):
    values = rand_values(colind.numel(), dtype, dev, 3)
    B = rand_values(k * n, dtype, dev, 4).view(k, n)
    C = torch.empty((m, n), dtype=dtype, device=dev)
    a = sp.csr_view(values, rowptr, colind, (m, k), colind.numel())
    info = sp.multiply_inspect(a, B, C)
    ms = timed(lambda: sp.multiply(info, a, B, C), args.steps, args.warmup)
    s = values.element_size()
    nbytes = colind.numel() * (4 + s) + (m + 1) * 4 + k * n * s + m * n * s
    rows = np.sort(rng.choice(m, 1024, replace=False))
    err = sample_error(rowptr, colind, values, B, C, False, rows)
    return {"case": name, "dtype": str(dtype).replace("torch.", ""), "n": n, "ms": round(ms, 4), "alg_bytes": nbytes,
            "frac_8TBs": round(nbytes / (ms * 1e-3) / HBM, 3), "max_rel_err_sampled": err}


def kernel_stats(args):
    out = tempfile.mkdtemp(prefix="bench_complex_prof_", dir=args.prof_dir)
    cmd = ["timeout", "-k", "10", str(args.prof_timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run",
           "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--steps", "5", "--warmup", "2",
           "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return {"error": f"rocprofv3 run exited {r.returncode}", "stderr_tail": r.stderr[-800:]}
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"error": "no kernel_stats.csv"}
    rows = []
    with open(files[0]) as f:
        for rec in csv.DictReader(f):
            rows.append({"kernel": rec.get("Name", "")[:90], "calls": int(rec.get("Calls", 0)),
                         "avg_ms": round(float(rec.get("AverageNs", 0)) * 1e-6, 4)})
    rows.sort(key=lambda d: -d["avg_ms"] * d["calls"])
    return rows[:30]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--prof-timeout", type=int, default=600)
    ap.add_argument("--prof-dir", default=None, help="where the rocprofv3 output goes (default: a temporary directory)")
    ap.add_argument("--inner", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    recs = []
    m = args.rows
    for shape, (rp, ci) in (("cfg2_uniform", uniform_csr(m, m, 10, dev, 7)), ("banded", banded_csr(m, 10, 64, dev, 8))):
        for dtype in (torch.complex64, torch.complex128, torch.float64, torch.float32):
            for plan in (False, True):
                for conj_a in ((False, True) if dtype.is_complex else (False,)):
                    recs.append(spmv_case(f"spmv_{shape}", rp, ci, m, m, dtype, conj_a, plan, args, dev, rng))
                    torch.cuda.empty_cache()
        del rp, ci
        torch.cuda.empty_cache()
    mm = 2_000_000 if args.rows >= 2_000_000 else args.rows
    rp, ci = uniform_csr(mm, mm, 32, dev, 9)
    recs.append(spmm_case("spmm_cfg3_A", rp, ci, mm, mm, 64, torch.complex128, args, dev, rng))
    torch.cuda.empty_cache()
    recs.append(spmm_case("spmm_cfg3_A", rp, ci, mm, mm, 128, torch.float64, args, dev, rng))
    del rp, ci
    torch.cuda.empty_cache()

    def ms_of(case, dtype, plan, conj=False):
        for r in recs:
            if r["case"] == case and r["dtype"] == dtype and r.get("plan", "") == plan and r.get("conj_a", False) == conj:
                return r["ms"]
        return None

    ratios = {}
    for shape in ("spmv_cfg2_uniform", "spmv_banded"):
        for plan in ("plan_free", "rowblock"):
            c32, f64, c32c = ms_of(shape, "complex64", plan), ms_of(shape, "float64", plan), ms_of(shape, "complex64", plan, True)
            c64, c64c = ms_of(shape, "complex128", plan), ms_of(shape, "complex128", plan, True)
            ratios[f"{shape}/{plan}"] = {"c32_over_f64": round(c32 / f64, 3), "c32_conj_over_plain": round(c32c / c32, 3),
                                         "c64_conj_over_plain": round(c64c / c64, 3)}
    mmr = [r for r in recs if r["case"] == "spmm_cfg3_A"]
    ratios["spmm_cfg3_A"] = {"c64_n64_over_f64_n128": round(mmr[0]["ms"] / mmr[1]["ms"], 3)}
    out = {"metric": "complex_spmv_spmm", "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "records": recs, "ratios": ratios}
    if args.rocprof and not args.inner:
        out["kernel_stats"] = kernel_stats(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
