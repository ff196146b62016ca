#!/usr/bin/env python3
"""Runs tests/test_gpu_pcg.py on the GPU and writes, per run (contraction-form) and ld, the largest |(B - A X) - R| / drift_bound, the
largest true relative residual ||B - A X|| / ||B|| at rtol 1e-5 and at 1e-7 and the block's step counts to profiles/pcg_error.json
(or the path given), with the wall time of the module. The test keeps the record; this only runs it in one process with
GLF_PCG_ERROR_JSON set.

    python tools/pcg_error.py [out.json]"""
import json
import os
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pcg_error.json")
    os.environ["GLF_PCG_ERROR_JSON"] = out
    t0 = time.time()
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_pcg.py")])
    wall = time.time() - t0
    if os.path.exists(out):
        rec = json.load(open(out))
        rec["module_wall_seconds"] = round(wall, 1)
        rec["pytest_exit_code"] = int(rc)
        json.dump(rec, open(out, "w"), indent=1)
        print("wrote %s (%.1f s)" % (out, wall))
    else:
        print("nothing written")
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
