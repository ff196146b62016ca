"""The power-of-two operand scale rule of the split-f16 contractions (csrc/scale_rule.hpp), which the device kernels and the host
launchers share: the stand-alone driver tools/scale_rule_host_main.cpp holds it against an independent statement in double precision
(std::frexp / std::ldexp) at every f32 exponent with the mantissas 1, 1 + 2^-23 and 2 - 2^-23, at 0, the smallest and largest
subnormal, FLT_MAX, Inf and NaN, each with nr = 1, 4, 304 and 1024 -- exact equality, since every float is a double. CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_make_scale_rule_check_runs_clean(tmp_path):
    """Built with the address and undefined-behaviour sanitizers; the binary goes to the test's own directory."""
    out = subprocess.run(["make", "-C", ROOT, "scale_rule_check", "SCALE_RULE_CHECK_BIN=%s" % (tmp_path / "scale_rule_host_check")],
                         capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "scale_rule_host_check: ok" in out.stdout
