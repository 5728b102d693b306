"""Child process of tests/test_gpu_tt_ladders.py: the entry-count and rows-against-tiles ladders of the transpose under
SPBLAS_GFX950_TRANSPOSE_XCD=0, which csrc/transpose.hip reads once per process (set by the parent in this process's
environment).  Prints "compared <cases> cases with the remap off" and exits 0; an assertion that fails ends it with a traceback
and status 1."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ladder_tt as T  # noqa: E402
import tt_ladder_run as R  # noqa: E402


def main():
    assert os.environ.get("SPBLAS_GFX950_TRANSPOSE_XCD") == "0", "the parent sets the knob"
    compared = 0
    for case in T.entry_cases() + T.row_cases():
        for vt in ("f32", "f64"):
            R.run_transpose(case, vt)
            compared += 1
    print(f"compared {compared} cases with the remap off")


if __name__ == "__main__":
    main()
