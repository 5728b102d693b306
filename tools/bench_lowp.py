"""16-bit SpMV / SpMM measurements (csrc/lowp.hip): fp32 against bf16 against fp16 on the same structures, one JSON line
on stdout.

Cases (device-event times, median of --steps after --warmup):
  SpMV at cfg2's shape (10 M x 10 M, 10 entries per row, columns uniform) and on a banded matrix of the same size (10
  entries per row within +-64 columns of the diagonal), plan-free and ROWBLOCK.
  SpMM at cfg3's shape (A 2 M x 2 M, 32 entries per row uniform, B 2 M x 128 row-major), inspected.
Every record: ms, algorithmic bytes (per entry 4 + s, per row 4 + s for the offsets and y, per column s for x -- s = 2 for
the 16-bit types, 4 for fp32; SpMM: per entry 4 + s, plus k * n * s for B and m * n * s for C), the fraction of 8 TB/s,
and the worst |y - ref| / sum |a x| over sampled rows against float64 on the host (the 16-bit results carry the one
rounding of the output: up to 2^-9 of |y| for bf16, 2^-12 for fp16).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import spblas_reference_amd as sp  # noqa: E402
from spblas_reference_amd import _capi  # noqa: E402

HBM = 8.0e12
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


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


def rand_values(count, dtype, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand(count, device=dev, generator=g) - 0.5).to(dtype)


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


def sample_error(rowptr, colind, values, x, y, rows):
    """worst |y - ref| / sum |a x| over the sampled rows, reference in float64 on the host"""
    rp = rowptr.cpu().numpy().astype(np.int64)
    lo, hi = rp[rows], rp[rows + 1]
    idx = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)])
    it = torch.from_numpy(idx).to(values.device)
    v = values[it].double().cpu().numpy()
    xv = x[colind[it].long()].double().cpu().numpy()  # (gathered on the device: only the sampled rows' operands travel)
    seg = np.repeat(np.arange(len(rows)), hi - lo)
    prod = v[:, None] * xv if xv.ndim == 2 else v * xv
    ref = np.zeros((len(rows),) + prod.shape[1:])
    np.add.at(ref, seg, prod)
    absr = np.zeros(ref.shape)
    np.add.at(absr, seg, np.abs(prod))
    got = y[torch.from_numpy(rows).to(y.device)].double().cpu().numpy()
    return float(np.max(np.abs(got - ref) / np.maximum(absr, 1e-300)))


def _name(dtype):
    return str(dtype).replace("torch.", "")


def spmv_case(name, rowptr, colind, m, n, dtype, plan, args, dev, rng):
    values = rand_values(colind.numel(), dtype, dev, 1)
    x = rand_values(n, dtype, dev, 2)
    y = torch.empty(m, dtype=dtype, device=dev)
    a = sp.csr_view(values, rowptr, colind, (m, n), colind.numel())
    info = sp.multiply_inspect(a, x, y, alg=_capi.SPMV_ROWBLOCK) if plan else None
    fn = (lambda: sp.multiply(info, a, x, y)) if plan else (lambda: sp.multiply(a, x, y))
    ms = timed(fn, args.steps, args.warmup)
    s = values.element_size()
    nbytes = colind.numel() * (4 + s) + (m + 1) * 4 + n * s + m * s
    rows = np.sort(rng.choice(m, 4096, replace=False))
    err = sample_error(rowptr, colind, values, x, y, rows)
    return {"case": name, "dtype": _name(dtype), "plan": "rowblock" if plan else "plan_free", "ms": round(ms, 4),
            "alg_bytes": nbytes, "frac_8TBs": round(nbytes / (ms * 1e-3) / HBM, 3), "max_rel_err_sampled": err}


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
    err = sample_error(rowptr, colind, values, B, C, rows)
    return {"case": name, "dtype": _name(dtype), "n": n, "ms": round(ms, 4), "alg_bytes": nbytes,
            "frac_8TBs": round(nbytes / (ms * 1e-3) / HBM, 3), "max_rel_err_sampled": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=10_000_000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    recs = []
    m = args.rows
    for shape, (rp, ci) in (("cfg2_uniform", uniform_csr(m, m, 10, dev, 7)), ("banded", banded_csr(m, 10, 64, dev, 8))):
        for dtype in DTYPES:
            for plan in (False, True):
                recs.append(spmv_case(f"spmv_{shape}", rp, ci, m, m, dtype, plan, args, dev, rng))
                torch.cuda.empty_cache()
        del rp, ci
        torch.cuda.empty_cache()
    mm = 2_000_000 if args.rows >= 2_000_000 else args.rows
    rp, ci = uniform_csr(mm, mm, 32, dev, 9)
    for dtype in DTYPES:
        recs.append(spmm_case("spmm_cfg3", rp, ci, mm, mm, 128, dtype, args, dev, rng))
        torch.cuda.empty_cache()
    del rp, ci
    torch.cuda.empty_cache()

    def ms_of(case, dtype, plan=""):
        for r in recs:
            if r["case"] == case and r["dtype"] == dtype and r.get("plan", "") == plan:
                return r["ms"]
        return None

    ratios = {}
    for shape in ("spmv_cfg2_uniform", "spmv_banded"):
        for plan in ("plan_free", "rowblock"):
            f32 = ms_of(shape, "float32", plan)
            ratios[f"{shape}/{plan}"] = {"bf16_over_f32": round(ms_of(shape, "bfloat16", plan) / f32, 3),
                                         "f16_over_f32": round(ms_of(shape, "float16", plan) / f32, 3)}
    f32 = ms_of("spmm_cfg3", "float32")
    ratios["spmm_cfg3"] = {"bf16_over_f32": round(ms_of("spmm_cfg3", "bfloat16") / f32, 3),
                           "f16_over_f32": round(ms_of("spmm_cfg3", "float16") / f32, 3)}
    out = {"metric": "lowp_spmv_spmm", "device": torch.cuda.get_device_name(0), "steps": args.steps, "records": recs,
           "ratios": ratios}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
