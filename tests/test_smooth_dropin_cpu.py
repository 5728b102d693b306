"""CPU test: include/spblas/vendor/gfx950/smooth_impl.hpp compiles inside the reference tree (g++ -fsyntax-only on
tests/compile_check/dropin_smooth_check.cpp, the way tests/test_aggregate_dropin_cpu.py compiles the aggregate check), operands
out of scope are "no matching function", and both host layers declare the calls."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/include"
CHECK = os.path.join(ROOT, "tests", "compile_check", "dropin_smooth_check.cpp")
CALLS = ["smooth_prolongator_inspect", "smooth_prolongator_structure", "smooth_prolongator"]


def test_both_host_layers_declare_the_calls():
    impl = os.path.join("include", "spblas", "vendor", "gfx950", "smooth_impl.hpp")
    for path in (os.path.join("include", "spblas_gfx950", "spblas.hpp"), impl):
        text = open(os.path.join(ROOT, path)).read()
        for name in CALLS:
            assert f" {name}(operation_info_t& info" in text, (path, name)
    assert "smooth_impl.hpp" in open(os.path.join(ROOT, "include", "spblas", "vendor", "gfx950", "gfx950.hpp")).read()
    calls = open(os.path.join(ROOT, "include", "spblas", "vendor", "gfx950", "detail", "backend_calls.hpp")).read()
    header = open(os.path.join(ROOT, "include", "spblas_gfx950.h")).read()
    for name in ("smooth_create", "smooth_destroy", "smooth_info", "smooth_structure", "smooth_values"):
        assert "spblas_gfx950_" + name + "(" in calls, name
        assert "int spblas_gfx950_" + name + "(" in header, name


def _compile(tmp_path, extra):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    from oracle.reference_build import compile_flags, patched_reference_headers
    scratch = patched_reference_headers(str(tmp_path / "patched"))
    return subprocess.run([gxx, "-fsyntax-only"] + extra + compile_flags(scratch) + [CHECK], capture_output=True, text=True)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
def test_dropin_smooth_compiles_inside_the_reference_tree(tmp_path):
    r = _compile(tmp_path, [])
    assert r.returncode == 0, "smooth_impl.hpp does not compile inside the reference tree:\n" + r.stderr[-6000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
@pytest.mark.parametrize("case", ["SPBLAS_SMOOTH_COMPLEX", "SPBLAS_SMOOTH_SCALED", "SPBLAS_SMOOTH_WIDE"])
def test_dropin_smooth_out_of_scope_operands_are_no_matching_function(tmp_path, case):
    r = _compile(tmp_path, ["-D" + case])
    assert r.returncode != 0
    assert "no matching function" in r.stderr
