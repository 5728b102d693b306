"""CPU test: include/spblas/vendor/gfx950/aggregate_impl.hpp compiles inside the reference tree (g++ -fsyntax-only on
tests/compile_check/dropin_aggregate_check.cpp, the way tests/test_multicolor_cpu.py compiles the permute check), operands out of
scope are "no matching function", and both host layers declare the calls."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/include"
CHECK = os.path.join(ROOT, "tests", "compile_check", "dropin_aggregate_check.cpp")
CALLS = ["aggregate", "aggregate_copy", "prolongator", "coarsen_inspect", "coarsen_structure", "coarsen"]


def test_both_host_layers_declare_the_calls():
    impl = os.path.join("include", "spblas", "vendor", "gfx950", "aggregate_impl.hpp")
    for path in (os.path.join("include", "spblas_gfx950", "spblas.hpp"), impl):
        text = open(os.path.join(ROOT, path)).read()
        for name in CALLS:
            assert f" {name}(operation_info_t& info" in text, (path, name)
    assert "aggregate_impl.hpp" in open(os.path.join(ROOT, "include", "spblas", "vendor", "gfx950", "gfx950.hpp")).read()
    calls = open(os.path.join(ROOT, "include", "spblas", "vendor", "gfx950", "detail", "backend_calls.hpp")).read()
    for name in ("aggregate_create", "aggregate_destroy", "aggregate_info", "aggregate_copy", "aggregate_prolongator",
                 "coarsen_create", "coarsen_destroy", "coarsen_info", "coarsen_structure", "coarsen_values"):
        assert "spblas_gfx950_" + name + "(" in calls, name


def _compile(tmp_path, extra):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    from oracle.reference_build import compile_flags, patched_reference_headers
    scratch = patched_reference_headers(str(tmp_path / "patched"))
    return subprocess.run([gxx, "-fsyntax-only"] + extra + compile_flags(scratch) + [CHECK], capture_output=True, text=True)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
def test_dropin_aggregate_compiles_inside_the_reference_tree(tmp_path):
    r = _compile(tmp_path, [])
    assert r.returncode == 0, "aggregate_impl.hpp does not compile inside the reference tree:\n" + r.stderr[-6000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
@pytest.mark.parametrize("case", ["SPBLAS_AGGREGATE_COMPLEX", "SPBLAS_AGGREGATE_SCALED", "SPBLAS_AGGREGATE_WIDE"])
def test_dropin_aggregate_out_of_scope_operands_are_no_matching_function(tmp_path, case):
    r = _compile(tmp_path, ["-D" + case])
    assert r.returncode != 0
    assert "no matching function" in r.stderr
