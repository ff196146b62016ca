#!/usr/bin/env python3
"""Runs tests/test_gpu_filter.py on the GPU and writes, per kernel and case, the derived gamma and the largest |error| / bound observed to
profiles/filter_error.json (or the path given), with the case count and the wall time of the module. The test keeps the record; this
only runs it in one process with GLF_FILTER_ERROR_JSON set.

    python tools/filter_error.py [out.json]"""
import json
import os
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Count:
    passed = failed = 0

    def pytest_runtest_logreport(self, report):
        if report.when == "call":
            self.passed += report.passed
            self.failed += report.failed


def main():
    out = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "filter_error.json")
    os.environ["GLF_FILTER_ERROR_JSON"] = out
    count = _Count()
    t0 = time.time()
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "--durations=8", os.path.join(ROOT, "tests", "test_gpu_filter.py")], plugins=[count])
    wall = time.time() - t0
    if os.path.exists(out):
        rec = json.load(open(out))
        rec["cases_passed"], rec["cases_failed"] = count.passed, count.failed
        rec["module_wall_seconds"] = round(wall, 1)
        rec["pytest_exit_code"] = int(rc)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import filter_ref
        filter_ref.dump_record(out, rec)
        print("wrote %s (%d passed, %d failed, %.1f s)" % (out, count.passed, count.failed, wall))
    else:
        print("nothing written")
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
