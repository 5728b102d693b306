"""-m gpu: what the row-length and column-count ladders (tests/test_gpu_ladders.py) do not reach in the 16-bit and complex
SpMV / SpMM kernels (csrc/value_kernels.hpp with the value policies of csrc/lowp.hip and csrc/complex.hip), through the C ABI.

Signs and specials, bit for bit.  A 3 x 4 matrix whose first row holds products that are -0 and sums to -0, whose second row
cancels (2 + -2) and whose third is 1.5; x / B and y / C hold -0, NaN and +-inf; alpha in {1, -1}, beta in {0, 1, -1}, for
complex values also beta = i and all four conj_flags.  Paths: plan-free, VECTOR plan and ROWBLOCK plan for SpMV; layout_right
with the wide row access (n = 8), layout_right with the element-wise access (n = 1; n = 8 with a leading dimension of 9) and
layout_left for SpMM; the scale-only path of a matrix without entries.  Which zero, which NaN and which infinity comes out
depends on how each kernel forms its products (a plain multiply can give -0, an FMA onto +0 cannot), on whether beta == 0 skips
the read of y, and on the order of the conjugations: none of it follows from a formula a test could restate without copying the
kernel.  So the expected words are a RECORDING: EXPECTED below holds, per value type and path, the output words of every
(conj_flags, alpha, beta) in the order of combos(), as base64 of the zlib-compressed little-endian words.  They were recorded
once on an MI355X from the build of the commit BEFORE the kernels of lowp.hip and complex.hip were merged into one family
(each file then held its own copy of the eight kernels), and the merged family has to reproduce them.  One property is asserted
as a condition on top of the recording: with beta == 0 no NaN comes out, whatever y / C held.

One long row through each plan.  A row of 2 * window + 1 entries among a few short ones, for each of the three row-block
windows (read from the sources: ladder.thresholds()), integer data (ladder.exact_spmv_data / exact_spmm_data): the ROWBLOCK
SpMV leaves a tail, one whole window and a head of one entry in the plan's part_tail / part_head and the fix-up adds them; an
SpMM with a plan (n = 1 and 3) sends the row through the long-row parts kernels.  Compared with the integer result exactly.

Status order.  Malformed calls with several defects at once, so that the ORDER of an entry point's checks decides the answer;
the expected statuses are literals read off the entry points (lowp_spmv answers op = T before it looks at the handle, the
complex entry checks conj_flags first and reports op = T only after the sizes, ...)."""
import base64
import ctypes
import zlib

import numpy as np
import pytest
import torch

import ladder
from spblas_reference_amd import _capi
from spblas_reference_amd.api import _Handle

pytestmark = pytest.mark.gpu

VTS = ["f16", "bf16", "c64", "c128"]
CAPI_VT = {"f16": _capi.F16, "bf16": _capi.BF16, "c64": _capi.C32, "c128": _capi.C64}
WINDOW = {"f16": "window_lowp", "bf16": "window_lowp", "c64": "window_c64", "c128": "window_c128"}
M, K = 3, 4
ROWPTR = [0, 2, 4, 5]
COLIND = [0, 1, 2, 3, 1]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def is_cplx(vt):
    return vt in ("c64", "c128")


def scalar(vt, z):
    """alpha / beta as the C ABI takes them: one float for 16-bit values, (re, im) of the value's precision for complex."""
    if not is_cplx(vt):
        return (ctypes.c_float * 1)(z.real)
    return ((ctypes.c_float if vt == "c64" else ctypes.c_double) * 2)(z.real, z.imag)


def combos(vt):
    """(conj_flags, alpha, beta) in the order of the recording."""
    if not is_cplx(vt):
        return [(0, complex(a), complex(b)) for a in (1, -1) for b in (0, 1, -1)]
    return [(f, complex(a), b) for f in range(4) for a in (1, -1) for b in (0j, 1 + 0j, -1 + 0j, 1j)]


def make(vt, re, im, dev):
    """A tensor of the value type from float64 parts; the signs of zeros survive (torch.complex, no arithmetic)."""
    dt = ladder.TORCH_OF[vt]
    re = torch.tensor(re, dtype=torch.float64)
    if not dt.is_complex:
        return re.to(dt).to(dev)
    return torch.complex(re, torch.tensor(im, dtype=torch.float64)).to(dt).to(dev)


NAN, INF = float("nan"), float("inf")
A_RE, A_IM = [1.0, -0.0, 1.0, 1.0, 0.5], [-0.0, 1.0, 0.0, -0.0, -0.5]
X_RE, X_IM = [-0.0, 3.0, 2.0, -2.0], [0.0, -0.0, -2.0, 2.0]
COL_SCALE = [1.0, -1.0, 2.0, -2.0, 1.0, -1.0, 0.5, -0.5]
C_RE, C_IM = [-0.0, NAN, INF, 1.0, -INF], [NAN, -0.0, 1.0, INF]


def operands(vt, n, dev):
    """(values, B as K x n, C0 as M x n) -- n = 1: x and y."""
    s = COL_SCALE[:n]
    B = make(vt, [[x * c for c in s] for x in X_RE], [[x * c for c in s] for x in X_IM], dev)
    C0 = make(vt, [[C_RE[(i + 2 * j) % 5] for j in range(n)] for i in range(M)],
              [[C_IM[(i + j) % 4] for j in range(n)] for i in range(M)], dev)
    return make(vt, A_RE, A_IM, dev), B, C0


def words(t):
    """The tensor's elements as unsigned little-endian words, row-major."""
    w = ladder.bits(t.cpu()).numpy().reshape(-1)
    return w.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[w.itemsize])


def decode(blob, like):
    return np.frombuffer(zlib.decompress(base64.b64decode(blob)), dtype=like.dtype.newbyteorder("<")).astype(like.dtype)


def encode(w):
    return base64.b64encode(zlib.compress(w.astype(w.dtype.newbyteorder("<")).tobytes(), 9)).decode()


SPMV_PATHS = {"free": None, "vector": _capi.SPMV_VECTOR, "rowblock": _capi.SPMV_ROWBLOCK}
# (n, layout of B and C, entries of A)
SPMM_PATHS = {"right_n1": (1, "right", True), "right_n8": (8, "right", True), "right_ld9_n8": (8, "right_ld+1", True),
              "left_n1": (1, "left", True), "left_n8": (8, "left", True),
              "empty_right_n1": (1, "right", False), "empty_right_n8": (8, "right", False),
              "empty_left_n1": (1, "left", False), "empty_left_n8": (8, "left", False)}
GROUPS = [f"spmv_{p}" for p in SPMV_PATHS] + ["spmv_empty"] + [f"spmm_{p}" for p in SPMM_PATHS]


def strided(flat, rows, cols, layout):
    """A rows x cols view of the given layout at the start of `flat`, and (row stride, column stride)."""
    pad = int(layout.split("+")[1]) if "+" in layout else 0
    rs, cs = (1, rows + pad) if layout.startswith("left") else (cols + pad, 1)
    return torch.as_strided(flat, (rows, cols), (rs, cs)), rs, cs


def run_group(vt, group, dev):
    """The output words of every combo of `group`, concatenated; asserts that beta == 0 leaves no NaN."""
    lib, hd, cvt = _capi.lib(), _Handle.current(dev), CAPI_VT[vt]
    rowptr = torch.tensor(ROWPTR, dtype=torch.int32, device=dev)
    colind = torch.tensor(COLIND, dtype=torch.int32, device=dev)
    zeros = torch.zeros(M + 1, dtype=torch.int32, device=dev)
    plan = ctypes.c_void_p()
    if group.startswith("spmv"):
        n, layout, filled = 1, "right", group != "spmv_empty"
        alg = SPMV_PATHS.get(group[5:])
    else:
        (n, layout, filled), alg = SPMM_PATHS[group[5:]], None
    values, B, C0 = operands(vt, n, dev)
    rp, nnz = (rowptr, len(COLIND)) if filled else (zeros, 0)
    if alg is not None:
        assert lib.spblas_gfx950_spmv_plan_create(hd.h, ctypes.byref(plan), M, K, nnz, ptr(rp), ptr(colind), ptr(values),
                                                  _capi.I32, cvt, alg) == _capi.SUCCESS
        info = (ctypes.c_int64 * 12)()
        assert lib.spblas_gfx950_plan_info(plan, info) == _capi.SUCCESS and info[0] == alg
        assert alg != _capi.SPMV_ROWBLOCK or info[1] == ladder.thresholds()[WINDOW[vt]]
    Bf = torch.zeros(K * (n + 1) + 8, dtype=B.dtype, device=dev)
    Bv, brs, bcs = strided(Bf, K, n, layout)
    Bv.copy_(B)
    out = []
    try:
        for flags, alpha, beta in combos(vt):
            Cf = torch.zeros(M * (n + 1) + 8, dtype=B.dtype, device=dev)
            Cv, crs, ccs = strided(Cf, M, n, layout)
            Cv.copy_(C0)
            al, be = scalar(vt, alpha), scalar(vt, beta)
            if layout == "right" and n == 8:  # the wide row access wants 16-byte aligned rows
                assert Bf.data_ptr() % 16 == 0 and Cf.data_ptr() % 16 == 0
            if group.startswith("spmv"):
                args = (hd.h, plan, _capi.OP_N, M, K, nnz, al, ptr(rp), ptr(colind), ptr(values), ptr(Bf), be, ptr(Cf),
                        _capi.I32, cvt)
                rc = lib.spblas_gfx950_spmv_conj(*args, flags) if is_cplx(vt) else lib.spblas_gfx950_spmv(*args)
            else:
                args = (hd.h, None, M, K, n, nnz, al, ptr(rp), ptr(colind), ptr(values), ptr(Bf), brs, bcs, be, ptr(Cf), crs,
                        ccs, _capi.I32, cvt)
                rc = (lib.spblas_gfx950_spmm_strided_conj(*args, flags) if is_cplx(vt)
                      else lib.spblas_gfx950_spmm_strided(*args))
            assert rc == _capi.SUCCESS, (group, flags, alpha, beta, rc)
            got = Cv.contiguous().cpu()
            if beta == 0:
                assert not bool(torch.isnan(torch.view_as_real(got) if got.dtype.is_complex else got.float()).any()), \
                    f"{vt} {group} conj={flags} alpha={alpha} beta=0: NaN in the output (y / C was read)"
            out.append(words(got))
    finally:
        if plan:
            torch.cuda.synchronize()
            lib.spblas_gfx950_plan_destroy(hd.h, plan)
    return np.concatenate(out)


# recorded on an MI355X from the parent of the commit that introduced csrc/value_kernels.hpp (see the module docstring)
EXPECTED = {
    "f16/spmv_free": "eNpjYAACOyCuY6gBk38YGoBwHxDDRQBnhAdl",
    "f16/spmv_vector": "eNpjYAACOyCuY6gBk38YGoBwHxDDRQBnhAdl",
    "f16/spmv_rowblock": "eNpjYAACOyCuY6gBk38YGoBwHxDDRQBnhAdl",
    "f16/spmv_empty": "eNpjYICCOoYaMPmHAUMEAEDcBOk=",
    "f16/spmm_right_n1": "eNpjYAACOyCuY6gBk38YGoBwHxDDRQBnhAdl",
    "f16/spmm_right_n8": "eNpjYCAA7Bj2MTgxHALTVgy7gCI1DH8Y6hhs8LIOANVDWAxAsgZI78HLOgJUD2E1EID7gCoPAV0EoncBXdQAtxsfywWonhT3OADVg1kAgNhC6Q==",
    "f16/spmm_right_ld9_n8": "eNpjYCAA7Bj2MTgxHALTVgy7gCI1DH8Y6hhs8LIOANVDWAxAsgZI78HLOgJUD2E1EID7gCoPAV0EoncBXdQAtxsfywWonhT3OADVg1kAgNhC6Q==",
    "f16/spmm_left_n1": "eNpjYAACOyCuY6gBk38YGoBwHxDDRQBnhAdl",
    "f16/spmm_left_n8": "eNpjYCAA7Bj2MTgxHALTVgy7gCI1DH8Y6hhs8LIOANVDWAxAsgZI78HLOgJUD2E1EID7gCoPAV0EoncBXdQAtxsfywWonhT3OADVg1kAgNhC6Q==",
    "f16/spmm_empty_right_n1": "eNpjYICCOoYaMPmHAUMEAEDcBOk=",
    "f16/spmm_empty_right_n8": "eNpjYCAZ1DD8YahjsCGSxQAka4D0HiJZg8w9AIkTLvk=",
    "f16/spmm_empty_left_n1": "eNpjYICCOoYaMPmHAUMEAEDcBOk=",
    "f16/spmm_empty_left_n8": "eNpjYCAZ1DD8YahjsCGSxQAka4D0HiJZg8w9AIkTLvk=",
    "bf16/spmv_free": "eNpjYGBgOGAPxPUN9WDyP0MDQ8OB/UAMFwEA1wgN9w==",
    "bf16/spmv_vector": "eNpjYGBgOGAPxPUN9WDyP0MDQ8OB/UAMFwEA1wgN9w==",
    "bf16/spmv_rowblock": "eNpjYGBgOGAPxPUN9WDyP0MDQ8OB/UAMFwEA1wgN9w==",
    "bf16/spmv_empty": "eNpjYICAA/UN9WDyPwOGCACNtAn5",
    "bf16/spmm_right_n1": "eNpjYGBgOGAPxPUN9WDyP0MDQ8OB/UAMFwEA1wgN9w==",
    "bf16/spmm_right_n8": "eNqVjsEJwEAIBLcz7cztzO3MqIT87iD6cMBBF7iXTOnu2mmeAINVRTuTAu2/BBajd3kmBcdfAu+tlLk60MxOBH6/j9T32/+TB+MvPdk9gZ0=",
    "bf16/spmm_right_ld9_n8": "eNqVjsEJwEAIBLcz7cztzO3MqIT87iD6cMBBF7iXTOnu2mmeAINVRTuTAu2/BBajd3kmBcdfAu+tlLk60MxOBH6/j9T32/+TB+MvPdk9gZ0=",
    "bf16/spmm_left_n1": "eNpjYGBgOGAPxPUN9WDyP0MDQ8OB/UAMFwEA1wgN9w==",
    "bf16/spmm_left_n8": "eNqVjsEJwEAIBLcz7cztzO3MqIT87iD6cMBBF7iXTOnu2mmeAINVRTuTAu2/BBajd3kmBcdfAu+tlLk60MxOBH6/j9T32/+TB+MvPdk9gZ0=",
    "bf16/spmm_empty_right_n1": "eNpjYICAA/UN9WDyPwOGCACNtAn5",
    "bf16/spmm_empty_right_n8": "eNpjYCAVNNQ3/P//v8EeN+tAPYIFpP831APl9uNmAdXDWQyDzD0AfG5jqQ==",
    "bf16/spmm_empty_left_n1": "eNpjYICAA/UN9WDyPwOGCACNtAn5",
    "bf16/spmm_empty_left_n8": "eNpjYCAVNNQ3/P//v8EeN+tAPYIFpP831APl9uNmAdXDWQyDzD0AfG5jqQ==",
    "c64/spmv_free": "eNpjYAABBwcGODhgD8T7gfg/ENcjcEM9VAxd/D92cRAfpIehAWj+AQgNNn8/1A5qmc8ANR/Z/dQ23wHN/ftpYP5o+A9A+AMA+27mYQ==",
    "c64/spmv_vector": "eNpjYAABBwcGODhgD8T7gfg/ENcjcEM9VAxd/D92cRAfpIehAWj+AQgNNn8/1A5qmc8ANR/Z/dQ23wHN/ftpYP5o+A9A+AMA+27mYQ==",
    "c64/spmv_rowblock": "eNpjYAABBwcGODhgD8T7gfg/ENcjcEM9VAxd/D92cRAfpIehAWj+AQgNNn8/1A5qmc8ANR/Z/dQ23wHN/ftpYP5o+A9A+AMA+27mYQ==",
    "c64/spmv_empty": "eNpjYMAFDvwH4noEbqiHiqGL/8cuDuKD9IyaP2r+4DUfAItsyXE=",
    "c64/spmm_right_n1": "eNpjYAABBwcGODhgD8T7gfg/ENcjcEM9VAxd/D92cRAfpIehAWj+AQgNNn8/1A5qmc8ANR/Z/dQ23wHN/ftpYP5o+A9A+AMA+27mYQ==",
    "c64/spmm_right_n8": "eNrtlg2OhCAMhXsUb0JvRm9Gb+Yuf/GBMO7MGKPZmjTodPJ40Q94RPFipjxqHrU8a3ne9V0ZA319Ra2ok8rlueI8qXjQjxVKxd76W55IfL6XdftN/XZf/Qv8hv8Tlwu1hnq+1ZjpEfinAP2JvzqP+AP/68R/yIVaQz3fakz1wP+ix/5xLnnhv/HU+3etdx3oDfsDvfSuIreVn5H36Es2rhPnsnGvPOkHWAdSQP5wrFxXziv3dR3s+oX7ug7e4p+v41/A/8In8c/X8U/gn9xJ/POF/HPeg9LadS/4p45v6vgf9UN7Dny9/8Mej+yzDvrdGXBX/gn8P5F/Af+P5F/zNyD3B/67fV67c2DXd3AOnLH/wx6P2Se9r77fnQF3zT8C/p+Yfwj8PzL/cP4Gix7kH8v/lv8t/1v+t/xv+d/yv+V/y/+W/y3//5P8/wNet9dX",
    "c64/spmm_right_ld9_n8": "eNrtlguOgzAMRH0UbhLfDN8svlna/MTUCcvuFqGiGskKYOQM8OIMUT6YqY5aR23X2q6HfGhjpLePXCvXKRHqXHmeEjzJ54gtci49YyWStZ5L2u7pup13/QL38DkJNbBWObf1bH6nHoF+ipA3tew8sh7oTzv6Yw2reahn83v1QP+ix/pRu6Tx+a7/5R2t/gB6sG6aaJ/Mi/XKt8rcdn7SXD/JxnXhXDbulXfyEdaBNJD/OXauO+ed+74Ohnzjvq+DP/HP1/EvoH/hk/jn6/gn0E/hJP75Qv659qCydsMP/JPhmwz/s3x83Qfe7v/Q45F91kne7AGfyj+B/jvyL6D/lvxr/QcUfsG/6fNq9oEhH2AfOKP/Q49H71O+l82bPeBT/Y+A/jv6HwL9t/Q/XP/Bogf+x/2/+3/3/+7/3f+7/3f/7/7f/b/7f/f/X+L/H4o4y1c=",
    "c64/spmm_left_n1": "eNpjYAABBwcGODhgD8T7gfg/ENcjcEM9VAxd/D92cRAfpIehAWj+AQgNNn8/1A5qmc8ANR/Z/dQ23wHN/ftpYP5o+A9A+AMA+27mYQ==",
    "c64/spmm_left_n8": "eNrtlguOgzAMRH0UbhLfDN8svlna/MTUCcvuFqGiGskKYOQM8OIMUT6YqY5aR23X2q6HfGhjpLePXCvXKRHqXHmeEjzJ54gtci49YyWStZ5L2u7pup13/QL38DkJNbBWObf1bH6nHoF+ipA3tew8sh7oTzv6Yw2reahn83v1QP+ix/pRu6Tx+a7/5R2t/gB6sG6aaJ/Mi/XKt8rcdn7SXD/JxnXhXDbulXfyEdaBNJD/OXauO+ed+74Ohnzjvq+DP/HP1/EvoH/hk/jn6/gn0E/hJP75Qv659qCydsMP/JPhmwz/s3x83Qfe7v/Q45F91kne7AGfyj+B/jvyL6D/lvxr/QcUfsG/6fNq9oEhH2AfOKP/Q49H71O+l82bPeBT/Y+A/jv6HwL9t/Q/XP/Bogf+x/2/+3/3/+7/3f+7/3f/7/7f/b/7f/f/X+L/H4o4y1c=",
    "c64/spmm_empty_right_n1": "eNpjYMAFDvwH4noEbqiHiqGL/8cuDuKD9IyaP2r+4DUfAItsyXE=",
    "c64/spmm_empty_right_n8": "eNrtktENgCAMBbsZo7WbwWZqIEIhFb81R9KEgN57mhP5+irHNSpi2vZ2jLOiY1+Xjef8XX0/tfGskKczY8frmcndP/S7c0w3/WXp4/NyG88KeTozdryemd/7+yzb/P+p09o/zd1LwAvvA16NS+M7wu4q+I//+I//+I//+I//+I//+I//+I//+I//+I//+I//P/X/BOWG2iw=",
    "c64/spmm_empty_left_n1": "eNpjYMAFDvwH4noEbqiHiqGL/8cuDuKD9IyaP2r+4DUfAItsyXE=",
    "c64/spmm_empty_left_n8": "eNrtktENgCAMBbsZo7WbwWZqIEIhFb81R9KEgN57mhP5+irHNSpi2vZ2jLOiY1+Xjef8XX0/tfGskKczY8frmcndP/S7c0w3/WXp4/NyG88KeTozdryemd/7+yzb/P+p09o/zd1LwAvvA16NS+M7wu4q+I//+I//+I//+I//+I//+I//+I//+I//+I//+I//P/X/BOWG2iw=",
    "c128/spmv_free": "eNpjYEAGHA4MWMEPeyi9H0r/h9L12OkP9WjqCKn/T5p6mDzMHoYGqPsPoPLh7t+P5o/B5n4GNPfjCv/B7n4HAuG/f4i4fzT9j6b/EZH+AUgMDPA=",
    "c128/spmv_vector": "eNpjYEAGHA4MWMEPeyi9H0r/h9L12OkP9WjqCKn/T5p6mDzMHoYGqPsPoPLh7t+P5o/B5n4GNPfjCv/B7n4HAuG/f4i4fzT9j6b/EZH+AUgMDPA=",
    "c128/spmv_rowblock": "eNpjYEAGHA4MWMEPeyi9H0r/h9L12OkP9WjqCKn/T5p6mDzMHoYGqPsPoPLh7t+P5o/B5n4GNPfjCv/B7n4HAuG/f4i4fzT9j6b/EZH+AUgMDPA=",
    "c128/spmv_empty": "eNpjYCAH/PgPpeux0x/q0dQRUv+fNPUweZg9o+4fdf+o+0fdP+p+Ut0PACUe7jE=",
    "c128/spmm_right_n1": "eNpjYEAGHA4MWMEPeyi9H0r/h9L12OkP9WjqCKn/T5p6mDzMHoYGqPsPoPLh7t+P5o/B5n4GNPfjCv/B7n4HAuG/f4i4fzT9j6b/EZH+AUgMDPA=",
    "c128/spmm_right_n8": "eNrtmDHSgyAQhSksUlp6G7iZ3kyPYmlJmY6/SGDCG3cWTH6GcZ7NDug6y0v8WJ4xn9fDmXy85eMJ7k9wX8t/Whivposr1hXrSdHm64rrSdGV5R8xrhBjXnjH+RX9nM/7cP7ccz6fR/298Jz0Pm/zKNWV5rX6tPzK+oyg/74K+Upd2nr8/KX+oVL/NY+azmp9Wn5lfaOg/7D9Rn9Jdx/K3o/6i7+jpr8V9JHqDYW6F65Xqi+ua3zrvyN/Qp3+ZjnndeL5cs77ydXlI+/TfrAAkBuPkdfIc+Q97gdaPvIe94N/47+7J/9HQf/BdcZ/d0/+G0H/3XbGf3dT/ru8D0r7rr3If6Pw2yj8L8wX+d9L/y/08RL3H1tZ/qGcA8j/i/0/6E/+N+7/QX/yv23/H7+D3f6I/0o/PynnAS0f+/20H/TS/wt9vOT7pP+Xkn8o5wD6Pxf7f9Cf/k/j/h/0p//Ttv+P38Gwfen/0P+n/0//n/yn/0//n/4//X/6//R/6P/T/6f/T/+f/j/5T/+f/j/9f/r/9P/p/9D/v5H//wfR8ePW",
    "c128/spmm_right_ld9_n8": "eNrtmDHSgyAQhSksUlp6G7iZ3kyPYmlJmY6/SGDCG3cWTH6GcZ7NDug6y0v8WJ4xn9fDmXy85eMJ7k9wX8t/Whivposr1hXrSdHm64rrSdGV5R8xrhBjXnjH+RX9nM/7cP7ccz6fR/298Jz0Pm/zKNWV5rX6tPzK+oyg/74K+Upd2nr8/KX+oVL/NY+azmp9Wn5lfaOg/7D9Rn9Jdx/K3o/6i7+jpr8V9JHqDYW6F65Xqi+ua3zrvyN/Qp3+ZjnndeL5cs77ydXlI+/TfrAAkBuPkdfIc+Q97gdaPvIe94N/47+7J/9HQf/BdcZ/d0/+G0H/3XbGf3dT/ru8D0r7rr3If6Pw2yj8L8wX+d9L/y/08RL3H1tZ/qGcA8j/i/0/6E/+N+7/QX/yv23/H7+D3f6I/0o/PynnAS0f+/20H/TS/wt9vOT7pP+Xkn8o5wD6Pxf7f9Cf/k/j/h/0p//Ttv+P38Gwfen/0P+n/0//n/yn/0//n/4//X/6//R/6P/T/6f/T/+f/j/5T/+f/j/9f/r/9P/p/9D/v5H//wfR8ePW",
    "c128/spmm_left_n1": "eNpjYEAGHA4MWMEPeyi9H0r/h9L12OkP9WjqCKn/T5p6mDzMHoYGqPsPoPLh7t+P5o/B5n4GNPfjCv/B7n4HAuG/f4i4fzT9j6b/EZH+AUgMDPA=",
    "c128/spmm_left_n8": "eNrtmDHSgyAQhSksUlp6G7iZ3kyPYmlJmY6/SGDCG3cWTH6GcZ7NDug6y0v8WJ4xn9fDmXy85eMJ7k9wX8t/Whivposr1hXrSdHm64rrSdGV5R8xrhBjXnjH+RX9nM/7cP7ccz6fR/298Jz0Pm/zKNWV5rX6tPzK+oyg/74K+Upd2nr8/KX+oVL/NY+azmp9Wn5lfaOg/7D9Rn9Jdx/K3o/6i7+jpr8V9JHqDYW6F65Xqi+ua3zrvyN/Qp3+ZjnndeL5cs77ydXlI+/TfrAAkBuPkdfIc+Q97gdaPvIe94N/47+7J/9HQf/BdcZ/d0/+G0H/3XbGf3dT/ru8D0r7rr3If6Pw2yj8L8wX+d9L/y/08RL3H1tZ/qGcA8j/i/0/6E/+N+7/QX/yv23/H7+D3f6I/0o/PynnAS0f+/20H/TS/wt9vOT7pP+Xkn8o5wD6Pxf7f9Cf/k/j/h/0p//Ttv+P38Gwfen/0P+n/0//n/yn/0//n/4//X/6//R/6P/T/6f/T/+f/j/5T/+f/j/9f/r/9P/p/9D/v5H//wfR8ePW",
    "c128/spmm_empty_right_n1": "eNpjYCAH/PgPpeux0x/q0dQRUv+fNPUweZg9o+4fdf+o+0fdP+p+Ut0PACUe7jE=",
    "c128/spmm_empty_right_n8": "eNrt1EEKgzAQBVBvlqOlN/NKWbqLi5aANcNYKZTC+5tAMHbyLW9Z5PfZ+mutz7XV437r8+e2Ot8feczfF50bv1+OazTX2M/my87fnO90zxKcT+bK7tPqzf6XpJ/ofutxzXpO58vO35zvdM/1O/1Hvbd+7f3v/4vwO2b9l6CfaN5+sfeL943mG32X+ffY+mf9C//5z3/+81/4z3/+85//wn/+85///Bf+85///Oe/8J///Oc//4X//Oc///kv/Oc///n/L/7vENju+w==",
    "c128/spmm_empty_left_n1": "eNpjYCAH/PgPpeux0x/q0dQRUv+fNPUweZg9o+4fdf+o+0fdP+p+Ut0PACUe7jE=",
    "c128/spmm_empty_left_n8": "eNrt1EEKgzAQBVBvlqOlN/NKWbqLi5aANcNYKZTC+5tAMHbyLW9Z5PfZ+mutz7XV437r8+e2Ot8feczfF50bv1+OazTX2M/my87fnO90zxKcT+bK7tPqzf6XpJ/ofutxzXpO58vO35zvdM/1O/1Hvbd+7f3v/4vwO2b9l6CfaN5+sfeL943mG32X+ffY+mf9C//5z3/+81/4z3/+85//wn/+85///Bf+85///Oe/8J///Oc//4X//Oc///kv/Oc///n/L/7vENju+w==",
}


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("vt", VTS)
def test_signs_and_specials_match_the_recording(gpu, vt, group):
    got = run_group(vt, group, gpu)
    want = decode(EXPECTED[f"{vt}/{group}"], got)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    if bad.size:
        per = got.size // len(combos(vt))
        raise AssertionError(f"{vt} {group}: {bad.size} words differ from the recording; first: " + "; ".join(
            f"combo {combos(vt)[i // per]} word {i % per}: got {int(got[i]):#x}, recorded {int(want[i]):#x}" for i in bad[:6]))


# ------------------------------------------------------------------------------------------------------- one long row
def long_row_matrix(win):
    lens = np.array([3, 0, 2 * win + 1, 5, 1, 40], dtype=np.int64)
    rowptr = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    colind = np.random.default_rng(win).integers(0, 64, int(rowptr[-1])).astype(np.int32)
    return rowptr, colind, (int(lens.size), 64)


def int_tensor(vt, shape, seed, dev):
    """Small integers (real and imaginary parts in -2 ... 2) of the value type, and the same as float64 / complex128 numpy."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-2, 3, shape).astype(np.float64)
    if is_cplx(vt):
        a = a + 1j * rng.integers(-2, 3, shape)
    return ladder.cast(vt, a).to(dev), a


@pytest.mark.parametrize("off", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("vt", VTS)
def test_one_long_row_through_the_rowblock_plan(gpu, vt, off):
    lib, hd, cvt = _capi.lib(), _Handle.current(gpu), CAPI_VT[vt]
    win = ladder.thresholds()[WINDOW[vt]]
    rowptr, colind, shape = long_row_matrix(win)
    values, x = ladder.exact_spmv_data(rowptr, colind, shape[1], cplx=is_cplx(vt), f16=vt == "f16")
    ref, _ = ladder.spmv_reference(rowptr, colind, values, x, shape)
    rp, ci = torch.as_tensor(rowptr).to(off).to(gpu), torch.as_tensor(colind).to(gpu)
    v, xd = ladder.cast(vt, values).to(gpu), ladder.cast(vt, x).to(gpu)
    y, y0 = int_tensor(vt, shape[0], 3, gpu)
    plan = ctypes.c_void_p()
    ot = _capi.I32 if off == torch.int32 else _capi.I64
    assert lib.spblas_gfx950_spmv_plan_create(hd.h, ctypes.byref(plan), shape[0], shape[1], colind.size, ptr(rp), ptr(ci),
                                              ptr(v), ot, cvt, _capi.SPMV_ROWBLOCK) == _capi.SUCCESS
    try:
        info = (ctypes.c_int64 * 12)()
        assert lib.spblas_gfx950_plan_info(plan, info) == _capi.SUCCESS
        assert (info[0], info[1], info[3], info[4]) == (_capi.SPMV_ROWBLOCK, win, 1, 2 * win + 1)
        args = (hd.h, plan, _capi.OP_N, shape[0], shape[1], colind.size, scalar(vt, 1 + 0j), ptr(rp), ptr(ci), ptr(v), ptr(xd),
                scalar(vt, 1 + 0j), ptr(y), ot, cvt)
        rc = lib.spblas_gfx950_spmv_conj(*args, 0) if is_cplx(vt) else lib.spblas_gfx950_spmv(*args)
        assert rc == _capi.SUCCESS
        ladder.check_exact(vt, y, ref + y0, f"{vt} long row, ROWBLOCK SpMV")
    finally:
        torch.cuda.synchronize()
        lib.spblas_gfx950_plan_destroy(hd.h, plan)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("vt", VTS)
def test_one_long_row_through_the_spmm_parts(gpu, vt, n):
    lib, hd, cvt = _capi.lib(), _Handle.current(gpu), CAPI_VT[vt]
    win = ladder.thresholds()[WINDOW[vt]]
    rowptr, colind, shape = long_row_matrix(win)
    values, B = ladder.exact_spmm_data(rowptr, colind, shape, 3, cplx=is_cplx(vt), f16=vt == "f16")
    B = np.ascontiguousarray(B[:, :n])
    ref, _ = ladder.spmm_reference(rowptr, colind, values, B, shape)
    rp, ci = torch.as_tensor(rowptr).to(torch.int32).to(gpu), torch.as_tensor(colind).to(gpu)
    v, Bd = ladder.cast(vt, values).to(gpu), ladder.cast(vt, B).to(gpu)
    C, C0 = int_tensor(vt, (shape[0], n), 4, gpu)
    plan = ctypes.c_void_p()
    assert lib.spblas_gfx950_spmv_plan_create(hd.h, ctypes.byref(plan), shape[0], shape[1], colind.size, ptr(rp), ptr(ci),
                                              ptr(v), _capi.I32, cvt, _capi.SPMV_AUTO) == _capi.SUCCESS
    try:
        info = (ctypes.c_int64 * 12)()
        assert lib.spblas_gfx950_plan_info(plan, info) == _capi.SUCCESS and (info[1], info[3]) == (win, 1)
        args = (hd.h, plan, shape[0], shape[1], n, colind.size, scalar(vt, 1 + 0j), ptr(rp), ptr(ci), ptr(v), ptr(Bd), n, 1,
                scalar(vt, 1 + 0j), ptr(C), n, 1, _capi.I32, cvt)
        rc = lib.spblas_gfx950_spmm_strided_conj(*args, 0) if is_cplx(vt) else lib.spblas_gfx950_spmm_strided(*args)
        assert rc == _capi.SUCCESS
        ladder.check_exact(vt, C, ref + C0, f"{vt} long row, SpMM with a plan, n = {n}")
    finally:
        torch.cuda.synchronize()
        lib.spblas_gfx950_plan_destroy(hd.h, plan)


# ------------------------------------------------------------------------------------------------------- status order
S = _capi
BIG = 2 ** 31  # an entry count that I32 offsets cannot hold


class Call:
    """The arguments of one well-formed multiply on the 3 x 4 matrix (n = 8 columns for SpMM); defects are set by name."""

    def __init__(self, vt, dev, plans):
        self.vt, self.cplx = vt, is_cplx(vt)
        self.values, self.B, self.C = operands(vt, 8, dev)
        self.rowptr = torch.tensor(ROWPTR, dtype=torch.int32, device=dev)
        self.colind = torch.tensor(COLIND, dtype=torch.int32, device=dev)
        self.plans = plans

    def args(self, hd, **d):
        a = dict(handle=hd.h, plan=None, op=S.OP_N, m=M, k=K, n=8, nnz=len(COLIND), alpha=scalar(self.vt, 1 + 0j),
                 rowptr=ptr(self.rowptr), colind=ptr(self.colind), values=ptr(self.values), B=ptr(self.B), brs=8, bcs=1,
                 beta=scalar(self.vt, 0j), C=ptr(self.C), crs=8, ccs=1, ot=S.I32, vt=CAPI_VT[self.vt], flags=0)
        a.update(d)
        return a

    def spmv(self, hd, conj, **d):
        a = self.args(hd, **d)
        lib = S.lib()
        base = (a["handle"], a["plan"], a["op"], a["m"], a["k"], a["nnz"], a["alpha"], a["rowptr"], a["colind"], a["values"],
                a["B"], a["beta"], a["C"], a["ot"], a["vt"])
        return lib.spblas_gfx950_spmv_conj(*base, a["flags"]) if conj else lib.spblas_gfx950_spmv(*base)

    def spmm(self, hd, entry, **d):
        a = self.args(hd, **d)
        lib = S.lib()
        head = (a["handle"], a["plan"], a["m"], a["k"], a["n"], a["nnz"], a["alpha"], a["rowptr"], a["colind"], a["values"], a["B"])
        if entry == "spmm":  # leading dimensions only
            return lib.spblas_gfx950_spmm(*head, a["brs"], a["beta"], a["C"], a["crs"], a["ot"], a["vt"])
        tail = (a["brs"], a["bcs"], a["beta"], a["C"], a["crs"], a["ccs"], a["ot"], a["vt"])
        if entry == "strided":
            return lib.spblas_gfx950_spmm_strided(*head, *tail)
        return lib.spblas_gfx950_spmm_strided_conj(*head, *tail, a["flags"])


# defects of an SpMV call -> status of (16-bit through spmv, complex through spmv and spmv_conj).  "other" is a plan of the
# same matrix made for another value type, None a null pointer / handle.  spmv_conj answers 16-bit values NOT_SUPPORTED
# before anything else (asserted for every row).
SPMV_TABLE = [
    (dict(op=S.OP_T, plan="other"), S.NOT_SUPPORTED, S.NOT_SUPPORTED),
    (dict(op=S.OP_T, handle=None), S.NOT_SUPPORTED, S.INVALID_HANDLE),
    (dict(op=S.OP_T, m=-1), S.NOT_SUPPORTED, S.INVALID_SIZE),
    (dict(op=S.OP_T, rowptr=None, C=None), S.NOT_SUPPORTED, S.NOT_SUPPORTED),
    (dict(op=S.OP_T, ot=7), S.NOT_SUPPORTED, S.INVALID_VALUE),
    (dict(m=-1, rowptr=None), S.INVALID_SIZE, S.INVALID_SIZE),
    (dict(handle=None, m=-1), S.INVALID_HANDLE, S.INVALID_HANDLE),
    (dict(nnz=BIG, rowptr=None, colind=None, values=None), S.INVALID_SIZE, S.INVALID_SIZE),
    (dict(nnz=BIG, ot=7), S.INVALID_VALUE, S.INVALID_VALUE),
    (dict(op=7, rowptr=None), S.INVALID_VALUE, S.INVALID_VALUE),
    (dict(B=None, plan="other"), S.INVALID_POINTER, S.INVALID_POINTER),
    (dict(plan="other"), S.PLAN_MISMATCH, S.PLAN_MISMATCH),
    (dict(plan="own", k=5), S.PLAN_MISMATCH, S.PLAN_MISMATCH),
    (dict(plan="own"), S.SUCCESS, S.SUCCESS),
]
# ... with conj_flags = 4 on top (spmv_conj only): complex values answer INVALID_VALUE whatever else is wrong
SPMV_FLAGS_TABLE = [dict(handle=None), dict(m=-1, rowptr=None), dict(op=S.OP_T), dict(plan="other"), dict()]

# defects of an SpMM call -> status, the same for 16-bit and complex values and for all three entries (spmm takes brs / crs as
# its leading dimensions and has no column strides: rows that set bcs / ccs are for the strided entries only)
SPMM_TABLE = [
    (dict(handle=None, brs=2, bcs=2), S.INVALID_HANDLE),
    (dict(handle=None, m=-1), S.INVALID_HANDLE),
    (dict(m=-1, rowptr=None), S.INVALID_SIZE),
    (dict(n=-1, C=None, ot=7), S.INVALID_SIZE),
    (dict(brs=2, bcs=2, ot=7, rowptr=None), S.INVALID_SIZE),                 # strides that are neither layout
    (dict(crs=3, ccs=2, plan="other"), S.INVALID_SIZE),
    (dict(brs=-1, bcs=8, plan="other"), S.INVALID_SIZE),
    (dict(brs=7, ot=7), S.INVALID_SIZE),                                     # layout_right, rows closer than n
    (dict(crs=7, C=None), S.INVALID_SIZE),
    (dict(nnz=BIG, rowptr=None, colind=None, values=None), S.INVALID_SIZE),
    (dict(nnz=BIG, ot=7, rowptr=None), S.INVALID_VALUE),
    (dict(ot=7, rowptr=None), S.INVALID_VALUE),
    (dict(B=None, plan="other"), S.INVALID_POINTER),
    (dict(C=None, plan="other"), S.INVALID_POINTER),
    (dict(plan="other"), S.PLAN_MISMATCH),
    (dict(plan="own", k=5), S.PLAN_MISMATCH),
    (dict(plan="own"), S.SUCCESS),
    # a B of ONE row: layout_left and layout_right are the same (strides (1, 1)), its row stride says nothing and is replaced
    # by n BEFORE the size check -- so brs = 1 < n is no INVALID_SIZE, and the next defect (or none) decides
    (dict(k=1, brs=1, nnz=0), S.SUCCESS),
    (dict(k=1, brs=1, nnz=0, C=None), S.INVALID_POINTER),
    (dict(k=1, brs=1, nnz=0, ot=7), S.INVALID_VALUE),
    (dict(m=1, crs=1, nnz=0, plan="own"), S.PLAN_MISMATCH),                  # ... and a C of one row
    (dict(m=1, crs=1, nnz=0, brs=7), S.INVALID_SIZE),
]
SPMM_FLAGS_TABLE = [dict(handle=None), dict(m=-1), dict(brs=2, bcs=2), dict(plan="other"), dict()]


@pytest.fixture(scope="module")
def calls(gpu):
    """A Call per value type, with a ROWBLOCK plan of its own type ("own") and one of another type ("other")."""
    lib, hd = _capi.lib(), _Handle.current(gpu)
    made, out = [], {}
    for vt in VTS:
        c = Call(vt, gpu, {})
        for name, pvt in (("own", vt), ("other", VTS[(VTS.index(vt) + 1) % 4])):
            p = ctypes.c_void_p()
            assert lib.spblas_gfx950_spmv_plan_create(hd.h, ctypes.byref(p), M, K, len(COLIND), ptr(c.rowptr), ptr(c.colind),
                                                      ptr(c.values), S.I32, CAPI_VT[pvt], S.SPMV_ROWBLOCK) == S.SUCCESS
            c.plans[name] = p
            made.append(p)
        out[vt] = c
    yield out
    torch.cuda.synchronize()
    for p in made:
        lib.spblas_gfx950_plan_destroy(hd.h, p)


def resolve(call, d):
    d = dict(d)
    if isinstance(d.get("plan"), str):
        d["plan"] = call.plans[d["plan"]]
    return d


@pytest.mark.parametrize("vt", VTS)
def test_status_order_spmv(gpu, calls, vt):
    c, hd = calls[vt], _Handle.current(gpu)
    for defects, lowp, cplx in SPMV_TABLE:
        d = resolve(c, defects)
        if c.cplx:
            assert c.spmv(hd, False, **d) == cplx, ("spmv", vt, defects)
            assert c.spmv(hd, True, **d) == cplx, ("spmv_conj", vt, defects)
        else:
            assert c.spmv(hd, False, **d) == lowp, ("spmv", vt, defects)
            assert c.spmv(hd, True, **d) == S.NOT_SUPPORTED, ("spmv_conj", vt, defects)
    for defects in SPMV_FLAGS_TABLE:
        want = S.INVALID_VALUE if c.cplx else S.NOT_SUPPORTED
        assert c.spmv(hd, True, flags=4, **resolve(c, defects)) == want, ("spmv_conj, conj_flags = 4", vt, defects)
    torch.cuda.synchronize()


@pytest.mark.parametrize("vt", VTS)
def test_status_order_spmm(gpu, calls, vt):
    c, hd = calls[vt], _Handle.current(gpu)
    for defects, want in SPMM_TABLE:
        d = resolve(c, defects)
        for entry in ("spmm", "strided", "strided_conj"):
            if entry == "spmm" and ("bcs" in d or "ccs" in d):
                continue
            w = S.NOT_SUPPORTED if entry == "strided_conj" and not c.cplx else want
            assert c.spmm(hd, entry, **d) == w, (entry, vt, defects)
    for defects in SPMM_FLAGS_TABLE:
        want = S.INVALID_VALUE if c.cplx else S.NOT_SUPPORTED
        assert c.spmm(hd, "strided_conj", flags=4, **resolve(c, defects)) == want, ("conj_flags = 4", vt, defects)
    torch.cuda.synchronize()
