"""Compiler evidence for the drop-in backend headers.

include/spblas/vendor/gfx950/*.hpp are the overloads a reference maintainer would compile in with
-DSPBLAS_ENABLE_GFX950.  The reference tree is only present in the build container, and its own headers need
range-v3 and kokkos-mdspan, which the image lacks.  This test
  1. copies the six reference headers INTEGRATION.md section 2 names into a scratch directory and applies exactly
     the edits that section lists (the scratch directory shadows the originals on the include path; nothing
     under /root/reference is written),
  2. puts tests/compile_check/stubs/ (a declared-only views::zip and a minimal rank-2 mdspan: COMPILE-CHECK
     infrastructure, they pin nothing and are not part of the product) where <range/v3/all.hpp> and
     <experimental/mdspan> are looked up,
  3. runs `g++ -std=c++20 -fsyntax-only -DSPBLAS_ENABLE_GFX950` on tests/compile_check/dropin_check.cpp, which
     instantiates every overload: multiply / multiply_inspect (SpMV on span, SpMM on row-major mdspan),
     multiply_compute / multiply_fill / multiply_symbolic_* / multiply_numeric (3- and 4-argument), add*,
     transpose*, scale, triangular_solve*.
Skipped where /root/reference does not exist (the GPU box).
"""
import os
import shutil
import subprocess

import pytest

import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference/include"
CHECK = os.path.join(ROOT, "tests", "compile_check")

pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")


from oracle.reference_build import compile_flags, patched_reference_headers  # noqa: E402


def test_dropin_headers_compile_inside_the_reference_tree(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    scratch = patched_reference_headers(str(tmp_path / "patched"))
    cmd = [gxx, "-fsyntax-only"] + compile_flags(scratch) + [os.path.join(CHECK, "dropin_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "drop-in headers do not compile inside the reference tree:\n" + r.stderr[-6000:]


def test_dropin_headers_log_through_the_reference_macros(tmp_path):
    """SURVEY.md section 5, metrics / logging: the reference's only instrumentation is the compile-time LOG_LEVEL printf
    (`detail/log.hpp:32-90`, `log_trace("")` at each entry of `algorithms/multiply_impl.hpp:21,36,69` and of the oneMKL
    backend).  Every public overload of this backend opens with the same `log_trace("")`; with -DLOG_LEVEL set the
    macros expand to real calls and must still compile."""
    gxx = shutil.which("g++")
    scratch = patched_reference_headers(str(tmp_path / "patched"))
    cmd = [gxx, "-fsyntax-only", "-DLOG_LEVEL=SPBLAS_INFO"] + compile_flags(scratch) + [os.path.join(CHECK, "dropin_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    n = 0
    for name in os.listdir(os.path.join(ROOT, "include", "spblas", "vendor", "gfx950")):
        if name.endswith(".hpp"):
            with open(os.path.join(ROOT, "include", "spblas", "vendor", "gfx950", name)) as f:
                n += f.read().count('log_trace("")')
    assert n >= 30, n


def test_cmake_module_configures_and_builds_the_backend():
    """cmake/SpblasGfx950.cmake (INTEGRATION.md section 2's CMake lines as a module) with -DENABLE_GFX950=ON: configure +
    build of tests/compile_check/cmake_project, which links dropin_run.cpp through the INTERFACE target `spblas` the way the
    reference's CMakeLists.txt:80-88 links its rocSPARSE slot.  (The binary runs on the GPU in tests/test_gpu_dropin.py.)"""
    import spblas_reference_amd as sp
    from oracle.reference_build import build_dropin_run_with_cmake
    if shutil.which("cmake") is None:
        pytest.skip("cmake not installed")
    if not os.path.exists(sp._build.LIBPATH):
        sp._build.build()
    binp = build_dropin_run_with_cmake(sp._build.LIBDIR)
    assert binp and os.path.exists(binp)
    needed = subprocess.run(["readelf", "-d", binp], capture_output=True, text=True).stdout
    assert "libspblas_gfx950.so" in needed and "rocsparse" not in needed
