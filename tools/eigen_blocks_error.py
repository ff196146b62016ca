#!/usr/bin/env python3
"""Runs the cases of tests/test_gpu_orthonormalise.py and tests/test_gpu_residual.py on the GPU and writes, per family (Gram-matrix
form and sweep by ld, panels, NormaliseVecs, sweep residual, derived residual, panels residual) and contraction mode, the largest
measured error, the tolerance or bound it is asserted against, their ratio and the emulation's d of that case to
profiles/eigen_blocks_error.json (or the path given). The tests keep the record (tests/eigen_ref.py, record / dump); this only runs
them in one process with GLF_EIGEN_ERROR_JSON set.

    python tools/eigen_blocks_error.py [out.json]"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "eigen_blocks_error.json")
    os.environ["GLF_EIGEN_ERROR_JSON"] = out
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_orthonormalise.py"),
                      os.path.join(ROOT, "tests", "test_gpu_residual.py")])
    print("wrote %s" % out if os.path.exists(out) else "nothing written")
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
