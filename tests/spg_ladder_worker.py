"""Child process of tests/test_gpu_spgemm_ladders.py: the EXACT three- and four-argument ladders of every family under knobs
that csrc/spgemm.hip reads once per process (SPBLAS_GFX950_SPG_DIRECT, _SPG_PACK, _SPG_RANKED_TPR, _SPG_RANKED_TPR1: set by
the parent in this process's environment).  Three numeric passes per state: by hash, by hash with recording, by rank.
Prints "compared <entries>" and exits 0; an assertion that fails ends it with a traceback and status 1."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ladder as L  # noqa: E402
import spg_ladder_run as R  # noqa: E402


def main():
    direct = os.environ.get("SPBLAS_GFX950_SPG_DIRECT", "1") != "0"
    vts = sys.argv[1].split(",") if len(sys.argv) > 1 else ["f32", "f64"]
    compared = 0
    for sub, aclass in L.spg_families():
        case = R.family_case(sub, aclass)
        for vt in vts:
            for addend in (False, True):
                compared += R.run_product(case, vt, True, addend, passes=3, classify_kw={"direct": direct})
    print(f"compared {compared}")


if __name__ == "__main__":
    main()
