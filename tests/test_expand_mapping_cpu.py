"""The block-to-thread mapping of the SLICED expand kernel (csrc/expand_map.hpp) on the host: tests/cpp/expand_map_check.cpp, a
stand-alone program with its own main, is compiled against the header with -fsanitize=address,undefined and run.  It
enumerates every range [b0, b1) with 0 <= b0 <= b1 <= 3 * L * 16 + 2 (L: the blocks a wavefront takes per iteration) for both
group widths -- 8 lanes per block (fp32) and 4 (fp64) -- and asserts that every block is handled by exactly one group exactly
once, that no table index outside the range is formed, and that the table words a wavefront reads in one iteration lie in one
aligned 128-byte line whenever b0 does.  The kernel calls the same function (asserted on the source)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spblas-reference_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "expand_map_check.cpp")


def _build(tmp_path, *flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "expand_map_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, *flags, SRC, "-o", exe], check=True, capture_output=True, text=True)
    return exe


def test_every_block_of_every_range_exactly_once(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), r.stdout + r.stderr
    # 3 * L * 16 + 2 = 770 (fp32, L = 16) and 1538 (fp64, L = 32): (n + 1)(n + 2) / 2 ranges each
    assert int(r.stdout.split()[1]) == 771 * 772 // 2 + 1539 * 1540 // 2, r.stdout


def test_the_check_bites(tmp_path):
    """The mapping of before (-DPB_EXP_FAR_PASS: the second window a workgroup pass behind the first) still covers every block
    once but reads a wavefront's table words from two lines: the program must say so."""
    r = subprocess.run([_build(tmp_path, "-DPB_EXP_FAR_PASS")], capture_output=True, text=True)
    assert r.returncode == 1 and "not consecutive" in r.stderr and "handled" not in r.stderr, r.stdout + r.stderr


def test_the_kernel_uses_the_header():
    src = open(os.path.join(CSRC, "spmv_sliced.hip")).read()
    body = src[src.index("void pb_expand_kernel("):src.index("pb_flag_dups_kernel")]
    assert '#include "expand_map.hpp"' in src
    assert re.search(r"const pb_exp_blocks m = pb_exp_map\(tid, it, b0, b1, LPB\);", body)
    # every table access of the kernel goes through the mapped blocks
    assert set(re.findall(r"blk(?:src|dst) \+ ([\w.]+)", body)) == {"m.a", "m.b"}
